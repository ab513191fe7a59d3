/**
 * bz2_fieldmatch.hip.h -- is field j of a line one of a set of values: the kernel under mi355x_bz2_match_fields, i.e.
 * under the reader's field_matches and select_lines.  bz2_fieldmatch.hpp has the definition (byte-for-byte equality with
 * one of the values; the key is only a filter) and the image of the value table.
 *
 * Nothing new is scanned.  The field-hash passes run as they are (bz2_fieldhash.hip.h) and leave key, start and size of the
 * field per closed line.  Then
 *
 *   k_field_match     grid-stride, one lane per line.  Every workgroup first copies the table's image to LDS -- the keys
 *                     sorted ascending, the offsets, the values' bytes: at most 8 + 4 + 16 KB --.  Per line: size < 0 (no
 *                     such field) gives 0; otherwise the lane binary-searches the line's key among the table's (at most
 *                     FIELDMATCH_STEPS steps), on a hit compares the sizes, and where they agree compares the field's
 *                     bytes, where they lie in the output, with the value's bytes in LDS.  One flag word per line: 1 or
 *                     0.  A span that does not lie inside the output's `outSize` bytes gives 0 and is never read.
 *
 * A start in `starts` is the field's offset in the output plus `delta` (mod 2^64): the C ABI's `base`, and for the
 * reader's one span the distance from the output to the file.  Places, offsets and line numbers are 64 bit.  Every loop is
 * bounded by FIELDMATCH_STEPS, by 256 or by the number of lines; no workgroup waits on another; plain vector loads and
 * stores.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bz2gpu
{
constexpr uint32_t FIELDMATCH_THREADS = 256, FIELDMATCH_BLOCKS = 512;
constexpr uint32_t FIELDMATCH_VALUES = 1024, FIELDMATCH_VALUE_BYTES = 256, FIELDMATCH_BYTES = 16384;
constexpr uint32_t FIELDMATCH_STEPS = 10;        /* 2^10 = FIELDMATCH_VALUES */
constexpr uint32_t FIELDMATCH_IMAGE_WORDS = ( FIELDMATCH_VALUES * 8 + ( FIELDMATCH_VALUES + 1 ) * 4 + FIELDMATCH_BYTES ) / 4;

/** keys[i], starts[i] and sizes[i] describe the field of line i of n; image[0, imageWords) is the table of k values,
 * 1 <= k <= FIELDMATCH_VALUES and imageWords <= FIELDMATCH_IMAGE_WORDS (the launcher checks both). */
__global__ __launch_bounds__( FIELDMATCH_THREADS ) void
k_field_match( const uint32_t* __restrict__ image, uint32_t imageWords, uint32_t k, const uint64_t* __restrict__ keys,
               const uint64_t* __restrict__ starts, const int64_t* __restrict__ sizes, uint64_t n, const uint8_t* __restrict__ out,
               uint64_t outSize, uint64_t delta, uint64_t* __restrict__ flags )
{
    /* uint64 for the alignment of the keys in front */
    __shared__ uint64_t table[( FIELDMATCH_IMAGE_WORDS + 1 ) / 2];
    uint32_t* const words = reinterpret_cast<uint32_t*>( table );
    for ( uint32_t w = threadIdx.x; w < imageWords; w += FIELDMATCH_THREADS ) words[w] = image[w];
    __syncthreads();
    const uint64_t* const tableKeys = table;
    const uint32_t* const offsets = words + 2 * k;
    const uint8_t* const bytes = reinterpret_cast<const uint8_t*>( offsets + k + 1 );

    for ( uint64_t i = (uint64_t)blockIdx.x * FIELDMATCH_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELDMATCH_THREADS ) {
        const int64_t size = sizes[i];
        uint64_t flag = 0;
        if ( size >= 0 && size <= (int64_t)FIELDMATCH_VALUE_BYTES ) {
            const uint64_t key = keys[i];
            /* the last table key that is not greater than `key`, if there is one: it is in [lo, hi), which halves from at
             * most 2^FIELDMATCH_STEPS to 1 */
            uint32_t lo = 0, hi = k;
            for ( uint32_t step = 0; step < FIELDMATCH_STEPS && hi - lo > 1; ++step ) {
                const uint32_t mid = ( lo + hi ) >> 1;
                if ( tableKeys[mid] <= key ) {
                    lo = mid;
                } else {
                    hi = mid;
                }
            }
            if ( tableKeys[lo] == key ) {
                const uint32_t from = offsets[lo], length = offsets[lo + 1] - from;
                const uint64_t at = starts[i] - delta;
                if ( length == (uint32_t)size && at <= outSize && (uint64_t)size <= outSize - at ) {
                    const uint8_t* const field = out + at;
                    uint32_t same = 0;
                    for ( ; same < length && same < FIELDMATCH_VALUE_BYTES; ++same ) {
                        if ( field[same] != bytes[from + same] ) break;
                    }
                    flag = same == length ? 1 : 0;
                }
            }
        }
        flags[i] = flag;
    }
}
}  // namespace bz2gpu
