/**
 * bz2_scratch.hpp -- the per-block scratch of a decoder context: ONE list of its regions, their sizes and the two pairs
 * that share memory.  Pure host arithmetic, no HIP: tests/native/scratch_cases.cpp pins the totals and checks that nothing
 * else overlaps.  bz2_device.hip makes one device and one page-locked host allocation of the totals and generates its
 * pointers from the same list; the kernel headers take their strides from here.
 */
#pragma once

#include <algorithm>
#include <cstdint>

#include "bz2_plan.hpp"   /* MAX_GROUPS, BWT_SPLIT_BLOCKS, BWT_SPLIT_MAX */

namespace bz2gpu
{
/* per block slot */
constexpr uint32_t L_STRIDE = 900096;         /* bytes per block in the L and R buffers (multiple of 256) */
constexpr uint32_t SEL_STRIDE = 32768;        /* bzip2.hpp:451 */
constexpr uint32_t TAB_STRIDE = 1u << 20;     /* u32 entries per block: every 20-bit index stays in bounds */
constexpr uint32_t KMAX = 32768;              /* max regular walk segments per block (+1 for origPtr) */
constexpr uint32_t SEG_STRIDE = KMAX + 64;
constexpr uint32_t STASH_BYTES = 128;         /* bytes of a segment the first walk keeps, see bz2_walk.hip.h */
constexpr uint32_t SYM_STRIDE = SEG_STRIDE * 64;   /* u16 per block: at most 900 100 symbols (n_sym <= N + 1), in a slot as large as the stash's */
constexpr uint32_t GPOS_STRIDE = 18048;       /* u32 per block: bit position of every 50-symbol group (k_hscan) */
constexpr int BWT_WAVES = 16;                 /* waves of a table-build workgroup (k_bwt_build) */
constexpr uint32_t BWT_COUNTS_PER_BLOCK = BWT_SPLIT_MAX * BWT_WAVES * 256;   /* u32 */

/** sizeof of the records that only device code knows, filled in by bz2_device.hip (which pins the values). */
struct ScratchSizes
{
    uint64_t blockMeta, huffMeta, scanMeta, huffTables, walkPlan;
};

enum ScratchMemory : bool { DEVICE = false, PINNED = true };   /* PINNED: page-locked host memory */

/* X( memory, name, element type, bytes, OWN or the region in whose memory it lives ), in the order in memory.  In scope of
 * the last two: n = block slots (size_t), s = ScratchSizes, keepStages. */
#define BZ2_SCRATCH_REGIONS( X )                                                                                              \
    X( DEVICE, dOffsets, uint64_t, n * sizeof( uint64_t ), OWN )                                                              \
    X( DEVICE, dOrder, uint32_t, n * sizeof( uint32_t ), OWN )                                                                \
    X( DEVICE, dMeta, BlockMeta, n * s.blockMeta, OWN )                                                                       \
    X( DEVICE, dSel, uint8_t, n * SEL_STRIDE + 256, OWN )                                                                     \
    X( DEVICE, dStb, uint8_t, n * 256, OWN )                                                                                  \
    X( DEVICE, dHmeta, HuffMeta, n * s.huffMeta, OWN )                                                                        \
    X( DEVICE, dSmeta, ScanMeta, n * s.scanMeta, OWN )               /* k_hscan -> k_hsym */                                  \
    X( DEVICE, dHtab, HuffTables, n * s.huffTables, OWN )            /* decode tables per block */                            \
    X( DEVICE, dGpos, uint32_t, n * GPOS_STRIDE * sizeof( uint32_t ), OWN )                                                   \
    X( DEVICE, dL, uint8_t, n * L_STRIDE + 256, OWN )                                                                         \
    X( DEVICE, dTab, uint32_t, n * TAB_STRIDE * sizeof( uint32_t ), OWN )                                                     \
    /* the bytes of the inverse BWT (k_emit -> k_rle) go where the block's last column was (k_mtf -> table build): same       \
     * slot, same stream, never alive together; 0.9 MB per block less.  Not when the caller wants to look at the stages */    \
    X( DEVICE, dR, uint8_t, n * L_STRIDE + 256, keepStages ? OWN : R_dL )                                                     \
    X( DEVICE, dSegLen, uint32_t, n * SEG_STRIDE * sizeof( uint32_t ), OWN )                                                  \
    X( DEVICE, dSegSucc, uint32_t, n * SEG_STRIDE * sizeof( uint32_t ), OWN )                                                 \
    X( DEVICE, dSegCont, uint32_t, n * SEG_STRIDE * sizeof( uint32_t ), OWN ) /* where a segment longer than STASH_BYTES goes on */ \
    X( DEVICE, dChain, uint2, n * SEG_STRIDE * 2 * sizeof( uint32_t ), OWN ) /* segments in cycle order {offset, length, segment} */ \
    X( DEVICE, dStash, uint32_t, n * SEG_STRIDE * STASH_BYTES, OWN ) /* first bytes of every segment */                       \
    /* the Huffman symbols of a block (k_hsym -> k_mtf) live where the block's stash will be (k_walk -> k_emit): same slot    \
     * size, never alive together, producers and consumers of a slot on one stream in that order; 1.8 MB per block less */    \
    X( DEVICE, dSym, uint16_t, n * SYM_STRIDE * sizeof( uint16_t ), R_dStash )                                                \
    X( DEVICE, dPlan, WalkPlan, MAX_GROUPS * s.walkPlan, OWN )       /* one per group */                                      \
    X( DEVICE, dWalkBlk, uint32_t, MAX_GROUPS * ( n + 16 ) * sizeof( uint32_t ), OWN )                                        \
    X( DEVICE, dWalkPre, uint32_t, MAX_GROUPS * ( n + 16 ) * sizeof( uint32_t ), OWN )                                        \
    X( DEVICE, dSlotOf, uint32_t, n * sizeof( uint32_t ), OWN )                                                               \
    X( DEVICE, dTotals, uint64_t, 2 * sizeof( uint64_t ), OWN )      /* k_offsets: {total decoded bytes, does not fit} */     \
    X( DEVICE, dBwtCounts, uint32_t, std::min<size_t>( n, BWT_SPLIT_BLOCKS ) * BWT_COUNTS_PER_BLOCK * sizeof( uint32_t ), OWN ) /* small batches */ \
    X( DEVICE, dEnds, uint64_t, n * sizeof( uint64_t ), OWN )        /* per-block end of the input, by slot */                \
    X( PINNED, hOrder, uint32_t, n * sizeof( uint32_t ), OWN )                                                                \
    X( PINNED, hSlotOf, uint32_t, n * sizeof( uint32_t ), OWN )      /* original index -> slot */                             \
    X( PINNED, hMeta, BlockMeta, n * s.blockMeta, OWN )                                                                       \
    X( PINNED, hOffsets, uint64_t, n * sizeof( uint64_t ), OWN )                                                              \
    X( PINNED, hTotals, uint64_t, 2 * sizeof( uint64_t ), OWN )                                                               \
    X( PINNED, hEnds, uint64_t, n * sizeof( uint64_t ), OWN )

static_assert( (size_t)SYM_STRIDE * sizeof( uint16_t ) == (size_t)SEG_STRIDE * STASH_BYTES );   /* dSym fills dStash's slot exactly */

enum ScratchRegion : int
{
#define BZ2_REGION_ID( memory, name, ... ) R_##name,
    BZ2_SCRATCH_REGIONS( BZ2_REGION_ID )
#undef BZ2_REGION_ID
    SCRATCH_REGIONS,
    OWN = -1   /* no other region's memory */
};

struct ScratchLayout
{
    uint32_t capacity{ 0 };                  /* block slots */
    uint64_t deviceBytes{ 0 }, hostBytes{ 0 };
    uint64_t offset[SCRATCH_REGIONS]{}, bytes[SCRATCH_REGIONS]{};
    bool host[SCRATCH_REGIONS]{};
    int aliasOf[SCRATCH_REGIONS]{};          /* the region whose memory this one lives in, or OWN */
};

/** Block slots for `nBlocks` (10 MB each): powers of two from 8 while that is cheap, multiples of 256 beyond 512. */
inline uint32_t
capacityFor( uint32_t nBlocks )
{
    uint32_t cap = 8;
    while ( cap < nBlocks && cap < 512 ) cap *= 2;
    return cap < nBlocks ? ( nBlocks + 255u ) & ~255u : cap;
}

/** Where every region of a context with `cap` block slots lies in its allocation, each at a multiple of 256 bytes. */
inline ScratchLayout
layScratch( uint32_t cap, bool keepStages, const ScratchSizes& s )
{
    ScratchLayout l;
    l.capacity = cap;
    const size_t n = cap;
    const auto place = [&l] ( int region, bool host, uint64_t bytes, int aliasOf ) {
        uint64_t& total = host ? l.hostBytes : l.deviceBytes;
        l.host[region] = host;
        l.bytes[region] = bytes;
        l.aliasOf[region] = aliasOf;
        l.offset[region] = aliasOf >= 0 ? l.offset[aliasOf] : total;
        if ( aliasOf < 0 ) total += ( bytes + 255 ) & ~uint64_t( 255 );
    };
#define BZ2_PLACE( memory, name, type, bytes, aliasOf ) place( R_##name, memory, bytes, aliasOf );
    BZ2_SCRATCH_REGIONS( BZ2_PLACE )
#undef BZ2_PLACE
    return l;
}
}  // namespace bz2gpu
