/* Ignoring case in the planner of the search (bz2_search.hpp) against a byte-by-byte restatement.
 *
 * foldAscii: all 256 bytes against a written-out table.
 *
 * seamMatches / seamMatchesSet with fold: a text is cut into extents back to back, every extent gives its first and last
 * min(m - 1, size) RAW bytes and nothing else, and the result must be exactly the matches of the whole text under the fold
 * -- restated here with a comparison that spells the 26 letters out -- that do not lie inside a single extent, ascending
 * and once each.  Extents of 1 to 3 bytes that a mixed-case match crosses several of; a match whose case differs from the
 * pattern's on both sides of a seam, asserted by name; m = 1; empty extents; patterns given in lower, upper and mixed case;
 * bytes next to the letters ('@', '[', '`', '{') and their counterparts above 0x80, which must not fold.  With the flag off
 * the same inputs must give what the exact functions give (and on text with mixed case that is less).  The same cuts once
 * more with the extents' file offsets shifted so that two extents meet exactly at 2^32, or one byte to either side.
 *
 * writeSetImage with fold: Err, eRR, err, [x and \xC5x land in the expected buckets, in id order, the stored bytes folded;
 * without fold the image is the exact one.  makePatternSet with fold changes neither ids, sizes nor m_min and m_max.
 * Prints "search fold ok". */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_search.hpp"

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

using Bytes = std::vector<uint8_t>;
using Patterns = std::vector<Bytes>;

/* the rule restated without arithmetic on the byte: the 26 pairs, written out */
uint8_t
lowerOf( uint8_t b )
{
    static const char upper[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZ", lower[] = "abcdefghijklmnopqrstuvwxyz";
    for ( int i = 0; i < 26; ++i ) {
        if ( b == (uint8_t)upper[i] ) return (uint8_t)lower[i];
    }
    return b;
}

bool
equalAt( const Bytes& text, uint64_t p, const Bytes& pattern, bool fold )
{
    for ( size_t j = 0; j < pattern.size(); ++j ) {
        const uint8_t a = text[p + j], b = pattern[j];
        if ( fold ? lowerOf( a ) != lowerOf( b ) : a != b ) return false;
    }
    return true;
}

Bytes
bytesOf( const char* s )
{
    return Bytes( s, s + std::strlen( s ) );
}

PatternSet
setOf( const Patterns& patterns, bool fold )
{
    Bytes all;
    std::vector<uint32_t> sizes;
    for ( const auto& pattern : patterns ) {
        all.insert( all.end(), pattern.begin(), pattern.end() );
        sizes.push_back( (uint32_t)pattern.size() );
    }
    return makePatternSet( all.data(), sizes.data(), sizes.size(), fold );
}

ExtentSeam
seamOf( const Bytes& text, uint64_t offset, uint64_t size, uint32_t m )
{
    const auto k = seamLength( m, size );
    return { offset, size, Bytes( text.begin() + offset, text.begin() + offset + k ),
             Bytes( text.begin() + offset + size - k, text.begin() + offset + size ) };
}

bool
insideOne( const std::vector<ExtentSeam>& seams, uint64_t p, uint64_t m )
{
    for ( const auto& seam : seams ) {
        if ( seam.fileOffset <= p && p + m <= seam.fileOffset + seam.size ) return true;
    }
    return false;
}

size_t seamMatchesSeen = 0, foldOnlySeen = 0;

/* both functions, fold on and off, for one cut of one text; `shift` is added to every extent's file offset, and so to
 * every expected position */
void
seamCase( const Bytes& text, const Patterns& patterns, const std::vector<uint64_t>& sizes, uint64_t from, uint64_t shift = 0 )
{
    uint64_t to = from;
    for ( const auto size : sizes ) to += size;
    CHECK( to <= text.size() );
    if ( to > text.size() ) return;
    uint32_t mMax = 0;
    for ( const auto& pattern : patterns ) mMax = std::max<uint32_t>( mMax, (uint32_t)pattern.size() );

    for ( const bool fold : { false, true } ) {
        /* single patterns */
        for ( const auto& pattern : patterns ) {
            const auto m = (uint32_t)pattern.size();
            std::vector<ExtentSeam> seams;
            uint64_t at = from;
            for ( const auto size : sizes ) {
                seams.push_back( seamOf( text, at, size, m ) );
                at += size;
            }
            std::vector<uint64_t> expected;
            for ( uint64_t p = from; p + m <= to; ++p ) {
                if ( equalAt( text, p, pattern, fold ) && !insideOne( seams, p, m ) ) expected.push_back( p );
            }
            for ( auto& seam : seams ) seam.fileOffset += shift;
            for ( auto& p : expected ) p += shift;
            const auto got = seamMatches( pattern.data(), m, seams, fold );
            CHECK( got == expected );
            if ( !fold ) CHECK( got == seamMatches( pattern.data(), m, seams ) );    /* the default is the exact search */
            if ( fold ) {
                seamMatchesSeen += got.size();
                foldOnlySeen += got.size() - seamMatches( pattern.data(), m, seams, false ).size();
            }
        }
        /* the set: made with the flag, and made without it and asked with it */
        std::vector<ExtentSeam> seams;
        uint64_t at = from;
        for ( const auto size : sizes ) {
            seams.push_back( seamOf( text, at, size, mMax ) );
            at += size;
        }
        std::vector<SetMatch> expected;
        for ( uint64_t p = from; p < to; ++p ) {
            for ( uint32_t i = 0; i < patterns.size(); ++i ) {
                const uint64_t m = patterns[i].size();
                if ( p + m <= to && equalAt( text, p, patterns[i], fold ) && !insideOne( seams, p, m ) ) expected.push_back( { p, i } );
            }
        }
        for ( auto& seam : seams ) seam.fileOffset += shift;
        for ( auto& pair : expected ) pair.first += shift;
        const auto made = setOf( patterns, fold );
        const auto plain = setOf( patterns, false );
        CHECK( made.fold == fold && made.sizes == plain.sizes && made.offsets == plain.offsets && made.bytes == plain.bytes
               && made.mMin == plain.mMin && made.mMax == plain.mMax && made.folded.size() == ( fold ? made.bytes.size() : 0 ) );
        CHECK( seamMatchesSet( made, seams ) == expected );
        CHECK( seamMatchesSet( plain, seams, fold ) == expected );
        CHECK( seamMatchesSet( made, seams, fold ) == expected );
        if ( !fold ) CHECK( seamMatchesSet( plain, seams ) == expected );
    }
}

void
foldTable()
{
    currentCase = "foldAscii, all 256 bytes";
    static const uint8_t table[256] = {
        0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F,
        0x10, 0x11, 0x12, 0x13, 0x14, 0x15, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x1B, 0x1C, 0x1D, 0x1E, 0x1F,
        0x20, 0x21, 0x22, 0x23, 0x24, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x2B, 0x2C, 0x2D, 0x2E, 0x2F,
        0x30, 0x31, 0x32, 0x33, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x3B, 0x3C, 0x3D, 0x3E, 0x3F,
        0x40, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x6B, 0x6C, 0x6D, 0x6E, 0x6F,
        0x70, 0x71, 0x72, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x5B, 0x5C, 0x5D, 0x5E, 0x5F,
        0x60, 0x61, 0x62, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x6B, 0x6C, 0x6D, 0x6E, 0x6F,
        0x70, 0x71, 0x72, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x7B, 0x7C, 0x7D, 0x7E, 0x7F,
        0x80, 0x81, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x8B, 0x8C, 0x8D, 0x8E, 0x8F,
        0x90, 0x91, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0x9B, 0x9C, 0x9D, 0x9E, 0x9F,
        0xA0, 0xA1, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xAB, 0xAC, 0xAD, 0xAE, 0xAF,
        0xB0, 0xB1, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xBB, 0xBC, 0xBD, 0xBE, 0xBF,
        0xC0, 0xC1, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF,
        0xD0, 0xD1, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xDB, 0xDC, 0xDD, 0xDE, 0xDF,
        0xE0, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xEB, 0xEC, 0xED, 0xEE, 0xEF,
        0xF0, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA, 0xFB, 0xFC, 0xFD, 0xFE, 0xFF,
    };
    for ( int b = 0; b < 256; ++b ) {
        CHECK( foldAscii( (uint8_t)b ) == table[b] );
        CHECK( lowerOf( (uint8_t)b ) == table[b] );    /* the restatement used below agrees with the table as well */
    }
    Bytes all( 256 );
    for ( int b = 0; b < 256; ++b ) all[b] = (uint8_t)b;
    CHECK( foldedBytes( all.data(), all.size(), true ) == Bytes( table, table + 256 ) );
    CHECK( foldedBytes( all.data(), all.size(), false ) == all );
}

/* `unit` repeated with every letter's case flipped with probability 1/2, and the neighbours of the letters sprinkled in */
Bytes
mixedText( size_t size, const Bytes& unit, std::mt19937_64& rng )
{
    static const uint8_t near[] = { '@', '[', '`', '{', 0xC1, 0xDA, 0xE1, 0xFA };
    Bytes text( size );
    for ( size_t i = 0; i < size; ++i ) {
        uint8_t b = unit[i % unit.size()];
        if ( ( ( b | 0x20 ) >= 'a' && ( b | 0x20 ) <= 'z' ) && ( rng() & 1 ) != 0 ) b ^= 0x20;
        text[i] = b;
    }
    for ( size_t k = 0; k < size / 61; ++k ) text[rng() % size] = near[rng() % sizeof( near )];
    return text;
}

void
seamCases()
{
    std::mt19937_64 rng( 0xF01D );
    const std::vector<Bytes> units{ bytesOf( "ab" ), bytesOf( "aBc" ), bytesOf( "Err0r[z{a@" ), bytesOf( "qZ\xC1\xE1z" ) };
    for ( const auto& unit : units ) {
        const Bytes text = mixedText( 6000, unit, rng );
        Bytes longLower( 40 ), longUpper( 40 ), longMixed( 40 );
        for ( size_t j = 0; j < 40; ++j ) {
            const uint8_t b = unit[j % unit.size()];
            const bool letter = ( b | 0x20 ) >= 'a' && ( b | 0x20 ) <= 'z' && b < 0x80;
            longLower[j] = letter ? (uint8_t)( b | 0x20 ) : b;
            longUpper[j] = letter ? (uint8_t)( b & ~0x20 ) : b;
            longMixed[j] = letter && ( j % 3 == 0 ) ? (uint8_t)( b ^ 0x20 ) : b;
        }
        const Patterns patterns{
            Bytes( longLower.begin(), longLower.begin() + 1 ),                                             /* m = 1 */
            Bytes( longUpper.begin(), longUpper.begin() + 2 ), Bytes( longLower.begin(), longLower.begin() + 2 ),   /* equal under the fold */
            Bytes( longMixed.begin(), longMixed.begin() + 5 ), Bytes( longUpper.begin(), longUpper.begin() + 3 ),   /* a prefix under the fold */
            longLower, longUpper, longMixed,
            { '[' }, { '{', 'a' }, { 0xE1, 'Z' }, { '@', 'A' },
        };
        currentCase = "extents of 1 to 3 bytes";
        std::vector<uint64_t> tiny;
        for ( int k = 0; k < 400; ++k ) tiny.push_back( 1 + rng() % 3 );
        seamCase( text, patterns, tiny, 3 );
        seamCase( text, patterns, std::vector<uint64_t>( 500, 1 ), 0 );
        seamCase( text, patterns, std::vector<uint64_t>( 300, 2 ), 1 );
        seamCase( text, patterns, std::vector<uint64_t>( 200, 3 ), 2 );
        currentCase = "empty extents between the others";
        seamCase( text, patterns, { 100, 0, 1, 0, 0, 2, 39, 0, 40, 41, 0, 3, 0, 500, 0 }, 17 );
        seamCase( text, patterns, { 0, 0, 0 }, 5 );
        seamCase( text, patterns, {}, 0 );
        seamCase( text, patterns, { 1000 }, 9 );
        currentCase = "extents that meet at 2^32, and next to it";
        for ( const uint64_t first : { (uint64_t)1000, (uint64_t)40, (uint64_t)1 } ) {
            const uint64_t cut = uint64_t( 1 ) << 32;
            for ( const uint64_t meet : { cut - 1, cut, cut + 1, cut + 39 } ) {
                seamCase( text, patterns, { first, 1000, 1, 2, 3, 1, 40, 0, 39, 500 }, 13, meet - 13 - first );
            }
        }
        currentCase = "seeded extent sizes";
        const std::vector<uint64_t> kinds{ 0, 1, 2, 3, 39, 40, 41, 137, 1000 };
        for ( int round = 0; round < 6; ++round ) {
            std::vector<uint64_t> sizes;
            for ( int k = 0; k < 12; ++k ) sizes.push_back( kinds[rng() % kinds.size()] );
            seamCase( text, patterns, sizes, rng() % 200 );
        }
    }
    currentCase = "coverage";
    CHECK( seamMatchesSeen > 1000 && foldOnlySeen > 500 );

    currentCase = "a match whose case differs on both sides of a seam";
    {
        const Bytes text = bytesOf( "..xxERror_lOG..Error_log.." );
        const Bytes pattern = bytesOf( "error_LOG" );
        /* [0,7) ends after "ERr": "ERr|or_lOG" has E and R on the left and l on the right in the other case than the
         * pattern; the second occurrence lies inside the last extent */
        const std::vector<uint64_t> sizes{ 7, 19 };
        std::vector<ExtentSeam> seams{ seamOf( text, 0, 7, 9 ), seamOf( text, 7, 19, 9 ) };
        CHECK( seamMatches( pattern.data(), 9, seams, true ) == std::vector<uint64_t>{ 4 } );
        CHECK( seamMatches( pattern.data(), 9, seams, false ).empty() );
        CHECK( seamMatches( pattern.data(), 9, seams ).empty() );
        /* across several extents of 1 to 3 bytes: 4 | 2 1 3 2 1 | 13 */
        seams = { seamOf( text, 0, 4, 9 ), seamOf( text, 4, 2, 9 ), seamOf( text, 6, 1, 9 ), seamOf( text, 7, 3, 9 ),
                  seamOf( text, 10, 2, 9 ), seamOf( text, 12, 1, 9 ), seamOf( text, 13, 13, 9 ) };
        CHECK( seamMatches( pattern.data(), 9, seams, true ) == std::vector<uint64_t>{ 4 } );
        const auto set = setOf( { bytesOf( "LOG" ), pattern, bytesOf( "Error" ), bytesOf( "r" ) }, true );
        seams = { seamOf( text, 0, 7, 9 ), seamOf( text, 7, 4, 9 ), seamOf( text, 11, 15, 9 ) };
        /* error_LOG at 4 crosses both ends, Error at 4 the first; lOG at 10 crosses the second; Error_log at 15 is inside */
        const std::vector<SetMatch> expected{ { 4, 1 }, { 4, 2 }, { 10, 0 } };
        CHECK( seamMatchesSet( set, seams ) == expected );
        CHECK( seamMatchesSet( setOf( { bytesOf( "LOG" ), pattern, bytesOf( "Error" ), bytesOf( "r" ) }, false ), seams ).empty() );
    }
    currentCase = "bytes that must not fold";
    {
        const Bytes text = bytesOf( "@a[a`a{a\xC1" "a\xE1" "a" );    /* 12 bytes */
        std::vector<ExtentSeam> seams;
        for ( uint64_t p = 0; p < 12; ++p ) seams.push_back( seamOf( text, p, 1, 2 ) );
        const auto matchesOf = [&] ( const char* pattern ) { return seamMatches( bytesOf( pattern ).data(), 2, seams, true ); };
        CHECK( matchesOf( "@A" ) == std::vector<uint64_t>{ 0 } && matchesOf( "`A" ) == std::vector<uint64_t>{ 4 } );
        CHECK( matchesOf( "[A" ) == std::vector<uint64_t>{ 2 } && matchesOf( "{A" ) == std::vector<uint64_t>{ 6 } );
        CHECK( matchesOf( "\xC1" "A" ) == std::vector<uint64_t>{ 8 } && matchesOf( "\xE1" "A" ) == std::vector<uint64_t>{ 10 } );
    }
}

void
imageCases()
{
    currentCase = "writeSetImage with fold";
    const Patterns patterns{ bytesOf( "Err" ), bytesOf( "[x" ), bytesOf( "eRR" ), bytesOf( "\xC5x" ), bytesOf( "err" ),
                             bytesOf( "E" ), bytesOf( "\xE5Y" ), bytesOf( "{" ), bytesOf( "Zz" ) };
    const auto set = setOf( patterns, true );
    std::vector<uint32_t> image( SET_IMAGE_BYTES / 4 + 1, 0xDEADBEEFu );
    auto* const bytes = reinterpret_cast<uint8_t*>( image.data() );
    writeSetImage( set, bytes, true );
    CHECK( image.back() == 0xDEADBEEFu );
    const uint32_t* const table = image.data() + SET_TABLE_AT / 4;
    const uint32_t* const first = image.data() + SET_FIRST_AT / 4;
    const auto bucket = [&] ( uint8_t byte ) {
        std::vector<uint32_t> ids;
        const uint32_t begin = first[byte] & 0xFFFFu, length = first[byte] >> 16;
        for ( uint32_t e = begin; e < begin + length; ++e ) {
            const uint32_t id = table[e] >> SET_ENTRY_ID_SHIFT, offset = table[e] & ( SET_MAX_BYTES - 1 );
            const uint32_t m = ( ( table[e] >> SET_ENTRY_SIZE_SHIFT ) & 0xFFu ) + 1;
            ids.push_back( id );
            CHECK( id < patterns.size() && m == patterns[id].size() && offset == set.offsets[id] );
            for ( uint32_t j = 0; j < m && id < patterns.size(); ++j ) CHECK( bytes[offset + j] == lowerOf( patterns[id][j] ) );
        }
        return ids;
    };
    CHECK( bucket( 'e' ) == ( std::vector<uint32_t>{ 0, 2, 4, 5 } ) );    /* Err, eRR, err, E: one bucket, id order */
    CHECK( bucket( '[' ) == std::vector<uint32_t>{ 1 } );
    CHECK( bucket( 0xC5 ) == std::vector<uint32_t>{ 3 } );
    CHECK( bucket( 0xE5 ) == std::vector<uint32_t>{ 6 } );                /* 0xC5 | 0x20, and a bucket of its own */
    CHECK( bucket( '{' ) == std::vector<uint32_t>{ 7 } );
    CHECK( bucket( 'z' ) == std::vector<uint32_t>{ 8 } );
    size_t entries = 0;
    for ( uint32_t byte = 0; byte < 256; ++byte ) {
        const uint32_t begin = first[byte] & 0xFFFFu, length = first[byte] >> 16;
        CHECK( ( first[byte] == 0 ) == ( length == 0 ) );
        CHECK( begin == ( length == 0 ? 0 : entries ) );    /* the buckets lie back to back in byte order */
        entries += length;
        if ( byte >= 'A' && byte <= 'Z' ) CHECK( first[byte] == 0 );
    }
    CHECK( entries == patterns.size() );

    currentCase = "writeSetImage without fold";
    std::vector<uint32_t> exact( SET_IMAGE_BYTES / 4 ), byDefault( SET_IMAGE_BYTES / 4 ), ofFoldedSet( SET_IMAGE_BYTES / 4 );
    writeSetImage( setOf( patterns, false ), reinterpret_cast<uint8_t*>( exact.data() ), false );
    writeSetImage( setOf( patterns, false ), reinterpret_cast<uint8_t*>( byDefault.data() ) );
    writeSetImage( set, reinterpret_cast<uint8_t*>( ofFoldedSet.data() ), false );
    CHECK( exact == byDefault && exact == ofFoldedSet );
    CHECK( std::memcmp( exact.data(), set.bytes.data(), set.bytes.size() ) == 0 );    /* the bytes as given */
    const uint32_t* const exactFirst = exact.data() + SET_FIRST_AT / 4;
    CHECK( ( exactFirst['E'] >> 16 ) == 2 && ( exactFirst['e'] >> 16 ) == 2 && ( exactFirst['Z'] >> 16 ) == 1 );
    /* a set made without the flag, written with it: the same image as the folded set's */
    std::vector<uint32_t> again( SET_IMAGE_BYTES / 4 );
    writeSetImage( setOf( patterns, false ), reinterpret_cast<uint8_t*>( again.data() ), true );
    CHECK( std::memcmp( again.data(), image.data(), SET_IMAGE_BYTES ) == 0 );
}
}  // namespace

int
main()
{
    foldTable();
    seamCases();
    imageCases();
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "search fold ok\n" );
    return 0;
}
