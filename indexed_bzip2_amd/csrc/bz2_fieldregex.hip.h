/**
 * bz2_fieldregex.hip.h -- does field j of a line match a regular expression: the kernel under
 * mi355x_bz2_match_fields_regex, i.e. under the reader's field_matches_regex and select_lines_regex.  bz2_fieldregex.hpp
 * has the definition (the table of bz2_regex.hpp run from state 0 over the field's bytes: A, or a state that accepts at
 * the end) and the dead state.
 *
 * Nothing new is scanned.  The field-span passes run as they are (bz2_fields.hip.h) and leave start and size of the field
 * per closed line.  Then
 *
 *   k_field_regex     grid-stride, one lane per line.  Every workgroup first copies the table and acceptsAtEnd to LDS
 *                     (loadRegexTable of bz2_regex.hip.h: at most 16 KiB + 64 B, so up to nine workgroups fit a CU by
 *                     LDS, and it is their waves that hide the dependent chain byte -> LDS -> state).  Per line: size
 *                     < 0 (no such field) gives 0; a span that does not lie inside the output's `outSize` bytes gives 0
 *                     and is never read; size 0 gives acceptsAtEnd[0]; otherwise the lane walks the field from state 0
 *                     and STOPS AT THE FIRST BYTE THAT LEADS TO A OR TO `dead`, the state from which no match can follow
 *                     (REGEX_STATES = REGEX_MAX_STATES, regexDeadState's answer, where there is none; the launcher
 *                     asserts that the two are equal): an anchored prefix pattern costs a few bytes per line, whatever
 *                     the field's length.  One flag word per line: 1 or 0.
 *
 * How a lane reads its field: in aligned 32-bit words, out of which it shifts the bytes, the next word already under way
 * while the current one is walked; no byte load per step.  The 64 fields of a wave lie in neighbouring lines, so their
 * words come from the same few cache lines step after step.  A word is loaded only if it holds a byte of the field, so it
 * begins in front of the output's end; that it also ENDS inside the buffer -- the last field of the output may end on the
 * output's last byte, and its last word reach up to 3 bytes behind it -- is established by ensureOutput's
 * `if ( size + 256 > buffer.capacity )` in bz2_device.hip (and by the same test in mi355x::resultBuffer for the result
 * buffer): 256 bytes of slack lie behind the output's bytes, and the buffers are hipMalloc's, aligned far beyond 16 bytes,
 * so an aligned word that begins inside the output lies inside the buffer.
 *
 * A wave runs as long as its longest field that is still walking, and a launch as long as its longest field: ONE lane
 * walks a field, at about 90 ns per byte (measured: profiles/fieldregex_probe.txt), 11 MB/s, whatever the rest of the grid
 * does.  A field of 64 KiB costs 6 ms, one of 4.5 MB -- the bench file holds such a line, a DNA sequence without a newline or
 * a blank -- 410 ms per launch, unless the pattern reaches A or the dead state early.  On fields of ordinary size the kernel
 * is a small part of the call.  Cutting a long field among the lanes of a wave needs the composition of bz2_regex.hip.h
 * (n-fold work for n states) and is not done here.
 *
 * A start in `starts` is the field's offset in the output plus `delta` (mod 2^64), as for k_field_match.  Places, offsets
 * and line numbers are 64 bit.  Every loop is bounded by the field's size or by the number of lines; no workgroup waits on
 * another; plain vector loads and stores.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_regex.hip.h"

namespace bz2gpu
{
constexpr uint32_t FIELDREGEX_THREADS = 256, FIELDREGEX_BLOCKS = 512;
static_assert( FIELDREGEX_THREADS == REGEX_THREADS, "loadRegexTable strides by REGEX_THREADS" );

/** starts[i] and sizes[i] describe the field of line i of n; table[nStates][256] and accepts[nStates] are the automaton,
 * 2 <= nStates <= REGEX_STATES (the launcher checks that); dead is regexDeadState's answer. */
__global__ __launch_bounds__( FIELDREGEX_THREADS ) void
k_field_regex( const uint8_t* __restrict__ table, const uint8_t* __restrict__ accepts, uint32_t nStates, uint32_t dead,
               const uint64_t* __restrict__ starts, const int64_t* __restrict__ sizes, uint64_t n, const uint8_t* __restrict__ out,
               uint64_t outSize, uint64_t delta, uint64_t* __restrict__ flags )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[REGEX_STATES * 256];
    __shared__ uint8_t ldsAccepts[REGEX_STATES];
    loadRegexTable( lds, ldsAccepts, table, accepts, nStates, threadIdx.x );

    for ( uint64_t i = (uint64_t)blockIdx.x * FIELDREGEX_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELDREGEX_THREADS ) {
        const int64_t size = sizes[i];
        uint64_t flag = 0;
        if ( size >= 0 ) {
            const uint64_t at = starts[i] - delta;
            if ( at <= outSize && (uint64_t)size <= outSize - at ) {
                uint32_t state = 0;
                if ( size > 0 ) {
                    /* the word that holds the field's first byte, then whole words; `have` bytes of `word` are unread,
                     * `left` bytes of the field are unwalked, and a word is loaded only if left > have: it holds one */
                    const uint32_t* from = reinterpret_cast<const uint32_t*>( out + ( at & ~uint64_t( 3 ) ) );
                    const uint32_t skip = (uint32_t)( at & 3 );
                    uint32_t word = *from >> ( 8 * skip ), have = 4 - skip;
                    uint64_t left = (uint64_t)size;
                    bool stop = false;
                    while ( !stop ) {
                        const bool more = left > have;
                        ++from;
                        const uint32_t next = more ? *from : 0u;
                        const uint32_t take = more ? have : (uint32_t)left;
                        for ( uint32_t k = 0; k < take; ++k ) {
                            state = lds[state * 256 + ( word & 0xFFu )];
                            word >>= 8;
                            if ( state == 1 || state == dead ) {
                                stop = true;
                                break;
                            }
                        }
                        if ( !more ) break;
                        left -= have;
                        word = next;
                        have = 4;
                    }
                }
                flag = ldsAccepts[state] != 0 ? 1 : 0;
            }
        }
        flags[i] = flag;
    }
}
}  // namespace bz2gpu
