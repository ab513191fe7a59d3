/**
 * bz2_mtf_expand.hpp -- what ONE symbol of a k_mtf chunk writes to the L column, as a rule that needs nothing but the
 * symbol's neighbourhood: plain integer functions for host and device, so that a CPU test (tests/native/mtf_expand_cases.cpp)
 * pins them against a byte-by-byte restatement of the serial loop.  k_mtf's pass B (bz2_stage1.hip.h) is this rule with
 * the three running values carried across the lanes of a wave.
 *
 * The symbols are those pass A leaves behind: a run digit stays 0 (RUNA) or 1 (RUNB), a literal is 2 + the POSITION its
 * entry has in the chunk's start list.
 *   - a literal writes one byte, list[s - 2];
 *   - the k-th digit (k = 0, 1, ...) of a digit sequence writes (s + 1) << k bytes -- the sum over a sequence is the serial
 *     loop's run length hh -- of the byte of the nearest literal before it in the chunk, list[0] if there is none.
 * Digit sequences never straddle chunks (the chunk rule moves the boundaries off them), so k is counted inside the chunk.
 * The serial loop keeps its digit weight in 32 bits: from 32 digits on it wraps and the rule no longer says what the loop
 * does.  Blocks with a sequence of more than MTF_EXPAND_MAX_DIGITS digits therefore stay with the serial loop, as do blocks
 * whose Huffman stage failed (an open run is then not flushed) and blocks that overflow the column.
 */
#pragma once

#include <cstdint>

#if defined( __HIPCC__ ) || defined( __CUDACC__ )
#define BZ2_MTF_HD __host__ __device__
#else
#define BZ2_MTF_HD
#endif

namespace bz2gpu
{
/** Longest digit sequence of a block that takes the data-parallel pass B: 20 digits are at least 2^20 - 1 bytes, more than
 * any column, and leave the 24 digits of history a lane looks back on (mtf_digit_index) and the 32-bit counts far from wrapping. */
constexpr uint32_t MTF_EXPAND_MAX_DIGITS = 20;

/** Pass A ORs the digit weight (1 << digits so far, the serial loop's runPos) after every digit into one word per lane. */
BZ2_MTF_HD inline bool
mtf_sequence_too_long( uint32_t weightsSeen )
{
    return ( weightsSeen >> ( MTF_EXPAND_MAX_DIGITS + 1 ) ) != 0;
}

/** Which blocks take the data-parallel pass B: for these neither overflow can occur (o + hh <= total <= maxN at every
 * flush, o < total at every literal) and every open run is flushed. */
BZ2_MTF_HD inline bool
mtf_expand_fast_path( bool huffmanOk, unsigned long long total, uint32_t maxN, bool sequenceTooLong, bool forceSerial )
{
    return huffmanOk && total <= maxN && !sequenceTooLong && !forceSerial;
}

/** `digits`: bit i set = symbol i is a run digit, for the 24 symbols in front of a group of eight (bits 0..23, the nearest at
 * bit 23) and the group itself (bits 24..31).  Returns how many digits stand directly in front of symbol j of the group:
 * its index k in its sequence.  Exact up to 24. */
BZ2_MTF_HD inline uint32_t
mtf_digit_index( uint32_t digits, uint32_t j )
{
    const uint32_t before = digits << ( 8u - j );      /* the symbol in front of j at bit 31; zeros come in from below */
    return (uint32_t)__builtin_clz( ~before );
}

/** Bytes that symbol s writes, k = digits directly in front of it. */
BZ2_MTF_HD inline uint32_t
mtf_expand_count( uint32_t s, uint32_t k )
{
    return s <= 1u ? ( s + 1u ) << k : 1u;
}

/** Position (in the chunk's start list) of the byte that symbol s writes; `lastLiteral` = that of the nearest literal
 * before it in the chunk, 0 (the list's front) if there is none.  It is the next symbol's `lastLiteral` as well. */
BZ2_MTF_HD inline uint32_t
mtf_expand_source( uint32_t s, uint32_t lastLiteral )
{
    return s <= 1u ? lastLiteral : s - 2u;
}
}  // namespace bz2gpu
