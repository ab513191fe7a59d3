/**
 * bz2_fieldcols.hpp -- a column of fields as bytes: field j of every line of a range, packed in line order, with the n + 1
 * offsets of the lines' fields and their n sizes (-1 where a line has no such field, which then owns no bytes).  The
 * definitions are bz2_fields.hpp's.  Host code only, no HIP: tests/native/fieldcols_cases.cpp pins it on the CPU.
 *
 * On one batch the GPU packs the fields that mi355x_bz2_field_spans found (bz2_fieldcols.hip.h, mi355x_bz2_gather_fields).
 * Over a file a column is assembled from STRETCHES, the resident pieces of the file that the launches of a line query
 * decode one after the other (bz2_linehash.hpp: planLineHashes, placeLineColumn).  A stretch packs the fields of the
 * lines it closes into a buffer of its own, with offsets local to it: its total is known only when its sizes are scanned.
 * The first closed line of a stretch that a line enters is computed "as if the stretch were entered at a line start"
 * (bz2_fields.hpp); stitchFields patches it, and what the stretch packed for it is not the field.  So the column is
 *
 *     for every stretch that holds wanted lines, in order:
 *         if its first wanted line is patched: the patched field, fetched from the file -- a FIX-UP --, and the stretch's
 *                                              pack from behind its first line's bytes on;
 *         else                                 the stretch's whole pack;
 *     then the patched unterminated tail, if the range reaches it: a fix-up.
 *
 * planColumnAssembly lays that out: the copies, the fix-ups and the final size.  A fix-up is a byte range of the decoded
 * file: there is one per line that crosses a seam between two launches (and the tail) and per field, and the blocks that
 * hold it are decoded a second time to fetch it.  That is the ONLY second decode of a column: every other block is decoded
 * once per call, whatever the number of fields.
 *
 * fieldColumn is the plain model of the whole column, straight from the definition.
 */
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace bz2gpu
{
constexpr uint32_t FIELD_COLUMNS_MAX = 16;            /* fields per call */
constexpr uint32_t FIELD_COLUMN_TILE_BYTES = 16384;   /* of k_field_gather, for mi355x_bz2_gather_fields_tile_bytes */

/** A stretch's place in the column's lines (ColumnPlace: lines [at, at + take) are its wanted ones), the bytes it packed
 * for them, and how many of those belong to the first of them. */
struct ColumnStretch
{
    uint64_t at{ 0 }, take{ 0 }, total{ 0 }, firstSize{ 0 };
};

/** A line the stitcher patched: its number in the column and its field in the file (size -1: missing). */
struct ColumnPatch
{
    uint64_t line{ 0 }, start{ 0 };
    int64_t size{ -1 };
};

struct ColumnCopy
{
    uint64_t stretch, src, dst, size;   /* bytes [src, src + size) of the stretch's pack to [dst, ...) of the column */

    [[nodiscard]] bool
    operator==( const ColumnCopy& o ) const
    {
        return stretch == o.stretch && src == o.src && dst == o.dst && size == o.size;
    }
};

struct ColumnFixup
{
    uint64_t fileOffset, size, dst;     /* bytes [fileOffset, fileOffset + size) of the decoded file to [dst, ...) */

    [[nodiscard]] bool operator==( const ColumnFixup& o ) const { return fileOffset == o.fileOffset && size == o.size && dst == o.dst; }
};

struct ColumnAssembly
{
    std::vector<ColumnCopy> copies;     /* ascending dst; none of size 0 */
    std::vector<ColumnFixup> fixups;    /* ascending dst; one per patched line with a present field, an empty one too */
    uint64_t size{ 0 };
};

/**
 * The rule of the header.  The stretches with take > 0 must tile the lines [0, closed) in order, and `patches` must
 * ascend by line, each naming the first wanted line of such a stretch or -- the last one only -- line `closed`, the
 * unterminated tail (checked: std::invalid_argument, as is a sum beyond 64 bits).  A stretch without wanted lines has
 * packed nothing.
 */
[[nodiscard]] inline ColumnAssembly
planColumnAssembly( const std::vector<ColumnStretch>& stretches, const std::vector<ColumnPatch>& patches )
{
    ColumnAssembly plan;
    const auto advance = [&plan] ( uint64_t bytes ) {
        if ( bytes > ~uint64_t( 0 ) - plan.size ) throw std::invalid_argument( "planColumnAssembly: the column overflows 64 bits" );
        plan.size += bytes;
    };
    const auto fix = [&] ( const ColumnPatch& patch ) {
        if ( patch.size < 0 ) return;
        plan.fixups.push_back( { patch.start, (uint64_t)patch.size, plan.size } );
        advance( (uint64_t)patch.size );
    };
    uint64_t closed = 0;
    size_t next = 0;
    for ( size_t k = 0; k < stretches.size(); ++k ) {
        const auto& s = stretches[k];
        if ( s.take == 0 ) {
            if ( s.total != 0 ) throw std::invalid_argument( "planColumnAssembly: stretch " + std::to_string( k ) + " packed bytes for no line" );
            continue;
        }
        if ( s.at != closed ) throw std::invalid_argument( "planColumnAssembly: stretch " + std::to_string( k ) + " does not follow the one in front of it" );
        if ( s.firstSize > s.total ) throw std::invalid_argument( "planColumnAssembly: the first line of stretch " + std::to_string( k ) + " is larger than its pack" );
        if ( next < patches.size() && patches[next].line < closed ) {
            throw std::invalid_argument( "planColumnAssembly: patch " + std::to_string( next ) + " names no stretch's first line" );
        }
        uint64_t src = 0;
        if ( next < patches.size() && patches[next].line == closed ) {
            fix( patches[next++] );
            src = s.firstSize;
        }
        if ( s.total > src ) {
            plan.copies.push_back( { k, src, plan.size, s.total - src } );
            advance( s.total - src );
        }
        closed += s.take;
    }
    if ( next < patches.size() && patches[next].line == closed ) fix( patches[next++] );
    if ( next != patches.size() ) throw std::invalid_argument( "planColumnAssembly: patch " + std::to_string( next ) + " names no stretch's first line" );
    return plan;
}

/** The whole column by the definition: data, offsets (n + 1) and sizes (n) of field j over the lines of bytes[0, size). */
struct FieldColumnModel
{
    std::vector<uint8_t> data;
    std::vector<uint64_t> offsets{ 0 };
    std::vector<int64_t> sizes;
};

[[nodiscard]] inline FieldColumnModel
fieldColumn( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j )
{
    FieldColumnModel column;
    size_t lineStart = 0;
    while ( lineStart < size ) {
        size_t lineEnd = lineStart;
        while ( lineEnd < size && bytes[lineEnd] != nl ) ++lineEnd;
        /* the j-th part of the content split at every dl */
        size_t partStart = lineStart;
        uint32_t part = 0;
        bool present = false;
        for ( size_t at = lineStart; at <= lineEnd; ++at ) {
            if ( at < lineEnd && bytes[at] != dl ) continue;
            if ( part == j ) {
                column.data.insert( column.data.end(), bytes + partStart, bytes + at );
                column.sizes.push_back( (int64_t)( at - partStart ) );
                present = true;
                break;
            }
            ++part;
            partStart = at + 1;
        }
        if ( !present ) column.sizes.push_back( -1 );
        column.offsets.push_back( column.data.size() );
        lineStart = lineEnd + 1;   /* behind the nl; an empty tail is no line */
    }
    return column;
}
}  // namespace bz2gpu
