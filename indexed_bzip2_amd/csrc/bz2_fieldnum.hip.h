/**
 * bz2_fieldnum.hip.h -- field j of every line as a number, for spans of a batch's ragged output: the kernels under
 * mi355x_bz2_field_numbers, i.e. under the reader's field_numbers and field_sums.  bz2_fieldnum.hpp has the definition
 * ([+-]?[0-9]{1,18}, else FIELD_NOT_A_NUMBER; FIELD_NUMBER_MISSING where the line has no such field) and the rule that
 * stitches stretches: an open line carries the first 19 bytes of its field and the field's size saturated at 20.
 *
 * Nothing new is scanned.  The passes of mi355x_bz2_field_spans run as they are (bz2_fields.hip.h: k_field_chunks,
 * k_field_link, k_scan_tiles, k_field_emit, k_field_sizes) and leave start and size of the field per closed line and, per
 * span, the head positions and the tail's field.  Then
 *
 *   k_field_numbers   grid-stride, one lane per closed line of [skip, skip + capacity): a missing field gives
 *                     FIELD_NUMBER_MISSING, an empty one or one of more than 19 bytes FIELD_NOT_A_NUMBER without a load;
 *                     otherwise the lane reads the field's 1 to 19 bytes where they lie in the output and parses them.
 *   k_field_texts     one workgroup per span, one lane per head segment and one for the tail: the FieldText -- size
 *                     saturated at 20, then the first 19 bytes -- of the bytes between two head positions (the span's
 *                     start in front of the first, the first nl or the span's end behind the last), field + 1 at the most,
 *                     and of the tail's field as far as the span reaches.
 *
 * A start in `starts` is the field's offset in the output plus `delta` (mod 2^64): 0 for the C ABI, and for the reader's
 * one span the distance from the output to the file.  Places, offsets and line numbers are 64 bit.  Every loop is bounded
 * by 20, by field + 2 or by the number of lines; no workgroup waits on another; plain vector loads and stores.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_fields.hip.h"

namespace bz2gpu
{
constexpr long long FIELDNUM_NOT_A_NUMBER = -0x7FFFFFFFFFFFFFFFll - 1;
constexpr long long FIELDNUM_MISSING = -0x7FFFFFFFFFFFFFFFll;
constexpr uint32_t FIELDNUM_BYTES = 19;          /* a sign and 18 digits */
constexpr uint32_t FIELDNUM_TEXT_BYTES = 20;     /* of a FieldText: its size, saturated at 20, and 19 bytes */
constexpr uint32_t FIELDNUM_TEXT_THREADS = 64;

/** A span for k_field_texts: where it lies in the output. */
struct FieldNumberSpan
{
    uint64_t offset, size;
};

/** The definition over bytes[0, size), 1 <= size <= 19. */
__device__ __forceinline__ long long
fnParse( const uint8_t* __restrict__ bytes, uint32_t size )
{
    const uint32_t first = bytes[0];
    const bool negative = first == '-', sign = negative || first == '+';
    if ( size - ( sign ? 1u : 0u ) - 1u >= 18u ) return FIELDNUM_NOT_A_NUMBER;      /* no digit, or more than 18 */
    long long value = 0;
    for ( uint32_t i = sign ? 1u : 0u; i < FIELDNUM_BYTES && i < size; ++i ) {
        const uint32_t digit = (uint32_t)bytes[i] - '0';
        if ( digit > 9u ) return FIELDNUM_NOT_A_NUMBER;
        value = value * 10 + digit;
    }
    return negative ? -value : value;
}

/** Behind k_field_sizes: starts[i] and sizes[i] hold field i of the closed lines [skip, skip + capacity).  The number of
 * closed lines is read where k_scan_tiles left it. */
__global__ __launch_bounds__( FIELD_SIZES_THREADS ) void
k_field_numbers( const uint64_t* __restrict__ places, const uint32_t* __restrict__ counts, uint64_t slots, uint64_t skip,
                 uint64_t capacity, const uint8_t* __restrict__ out, uint64_t delta, const uint64_t* __restrict__ starts,
                 const int64_t* __restrict__ sizes, long long* __restrict__ numbers )
{
    const uint64_t total = places[slots - 1] + counts[slots - 1];
    const uint64_t n = total > skip ? ( total - skip < capacity ? total - skip : capacity ) : 0;
    for ( uint64_t i = (uint64_t)blockIdx.x * FIELD_SIZES_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELD_SIZES_THREADS ) {
        const int64_t size = sizes[i];
        long long number = FIELDNUM_NOT_A_NUMBER;
        if ( size < 0 ) {
            number = FIELDNUM_MISSING;
        } else if ( size > 0 && size <= (int64_t)FIELDNUM_BYTES ) {
            number = fnParse( out + ( starts[i] - delta ), (uint32_t)size );
        }
        numbers[i] = number;
    }
}

/** The FieldText of out[from, to) to text[0, 20). */
__device__ __forceinline__ void
fnText( const uint8_t* __restrict__ out, uint64_t from, uint64_t to, uint8_t* __restrict__ text )
{
    const uint64_t size = to > from ? to - from : 0;
    text[0] = (uint8_t)( size < FIELDNUM_TEXT_BYTES ? size : FIELDNUM_TEXT_BYTES );
    for ( uint32_t i = 0; i < FIELDNUM_BYTES; ++i ) text[1 + i] = i < size ? out[from + i] : (uint8_t)0;
}

/** Behind k_field_link and k_field_emit, which completed the spans' summaries and head positions. */
__global__ __launch_bounds__( FIELDNUM_TEXT_THREADS ) void
k_field_texts( const FieldNumberSpan* __restrict__ extents, const FieldSpanSummary* __restrict__ spanSummaries,
               const uint64_t* __restrict__ headPositions, const uint8_t* __restrict__ out, uint32_t field,
               uint8_t* __restrict__ headTexts, uint8_t* __restrict__ tailTexts )
{
    const uint32_t cap = field + 1;
    const FieldNumberSpan extent = extents[blockIdx.x];
    const FieldSpanSummary s = spanSummaries[blockIdx.x];
    const uint64_t* const heads = headPositions + (uint64_t)blockIdx.x * cap;
    const uint32_t delims = s.headDelims < cap ? s.headDelims : cap;
    const uint32_t nTexts = delims + 1 < cap ? delims + 1 : cap;
    const uint64_t headEnd = ( s.info & FIELD_HAS_DELIMITER ) != 0 ? s.firstNl : extent.size;
    for ( uint32_t k = threadIdx.x; k < field + 2; k += FIELDNUM_TEXT_THREADS ) {
        if ( k == cap ) {
            const bool reached = s.tailFieldStart != FIELD_NOT_REACHED;
            const uint64_t from = reached ? s.tailFieldStart : 0;
            const uint64_t to = !reached ? 0 : ( s.tailFieldEnd != FIELD_NOT_REACHED ? s.tailFieldEnd : extent.size );
            fnText( out, extent.offset + from, extent.offset + to, tailTexts + (uint64_t)blockIdx.x * FIELDNUM_TEXT_BYTES );
        } else if ( k < nTexts ) {
            const uint64_t from = k == 0 ? 0 : heads[k - 1] + 1;
            const uint64_t to = k < delims ? heads[k] : headEnd;
            fnText( out, extent.offset + from, extent.offset + to, headTexts + ( (uint64_t)blockIdx.x * cap + k ) * FIELDNUM_TEXT_BYTES );
        }
    }
}
}  // namespace bz2gpu
