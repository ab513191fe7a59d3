/* The batch plan (bz2_plan.hpp) against the choices the launcher made before the plan was a function of its own: group
 * layout, scan form per group, k_mtf form, table-build slices and walk geometry, for batch sizes on both sides of every
 * threshold, with and without a crowd, uniform blocks and an expensive minority, and the test overrides.  Every case also
 * checks the slot invariants the kernels rely on.  Prints "plan ok". */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_plan.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            std::printf( "FAILED line %d (n = %u): %s\n", __LINE__, c.n, #cond );              \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

struct Case
{
    uint32_t n;
    uint64_t cheapBits;       /* compressed size of an ordinary block */
    uint32_t nExpensive;      /* blocks of 6 000 000 bits, spread evenly over the batch */
    bool crowd;
    PlanOverrides knobs;
    /* expected */
    int groups, expensive;
    uint32_t count[MAX_GROUPS];
    uint32_t scanWaves[MAX_GROUPS];
    bool mtfSide;
    uint32_t mtfSmallLanes, bwtSlices, walkWgsPerXcd, walkChunk;
};

/* the offsets of a batch laid out back to back; the input ends behind the last block */
std::vector<uint64_t>
layout( const Case& c, uint64_t* inSizeBytes )
{
    std::vector<uint64_t> offsets( c.n );
    uint64_t at = 0;
    for ( uint32_t i = 0; i < c.n; ++i ) {
        offsets[i] = at;
        const bool expensive = (uint64_t)( i + 1 ) * c.nExpensive / c.n > (uint64_t)i * c.nExpensive / c.n;
        at += expensive ? 6000000 : c.cheapBits;
    }
    *inSizeBytes = at / 8;
    return offsets;
}

/* Read off the launcher's code as it was before the plan moved here (n, bits per ordinary block, expensive blocks, crowd,
 * overrides {scan waves, table-build slices, narrow k_mtf, no split}; groups, expensive group, blocks per group, waves per
 * group, side stream, lanes of k_mtf<144>, slices, walk workgroups per XCD, segments per claim). */
const Case CASES[] = {
    /* uniform blocks of 6 000 000 bits: n at both sides of every threshold, one or two contexts, then a crowd */
    { 1, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 63, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 63, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 64, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 64, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 128, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 128, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 8, 128, 256 },
    { 129, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 129, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 4, 128, 256 },
    { 256, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 256, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 4, 128, 256 },
    { 257, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 257, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 384, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 384, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 385, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 385, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 640, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 640, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 641, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 641, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 128, 256 },
    { 800, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 800, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 128, 256 },
    { 801, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 801, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 128, 256 },
    { 1280, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 1280, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 128, 256 },
    { 1281, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 1281, 0, 0, 0 }, { 1, 0, 0, 0 }, false, 256, 1, 128, 256 },
    { 2560, 6000000, 0, false, { 0, 0, false, false }, 3, -1, { 426, 854, 1280, 0 }, { 1, 1, 1, 0 }, false, 256, 1, 128, 256 },
    { 1, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 63, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 63, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 64, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 64, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 128, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 128, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 8, 32, 256 },
    { 129, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 129, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 512, 4, 32, 256 },
    { 256, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 256, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 512, 4, 32, 1024 },
    { 257, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 257, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 2, 32, 1024 },
    { 384, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 384, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 2, 32, 1024 },
    { 385, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 385, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 2, 32, 1024 },
    { 640, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 640, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 2, 32, 1024 },
    { 641, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 641, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 32, 1024 },
    { 800, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 800, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 32, 1024 },
    { 801, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 801, 0, 0, 0 }, { 1, 0, 0, 0 }, true, 256, 1, 32, 1024 },
    { 1280, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 1280, 0, 0, 0 }, { 1, 0, 0, 0 }, true, 256, 1, 32, 1024 },
    { 1281, 6000000, 0, true, { 0, 0, false, false }, 1, -1, { 1281, 0, 0, 0 }, { 1, 0, 0, 0 }, false, 256, 1, 32, 1024 },
    { 2560, 6000000, 0, true, { 0, 0, false, false }, 3, -1, { 426, 854, 1280, 0 }, { 1, 1, 1, 0 }, false, 256, 1, 32, 1024 },
    /* a 20 % minority of expensive blocks (6 000 000 bits among blocks of 1 500 000) */
    { 1, 1500000, 0, false, { 0, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 63, 1500000, 12, false, { 0, 0, false, false }, 1, -1, { 63, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 64, 1500000, 12, false, { 0, 0, false, false }, 1, -1, { 64, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 128, 1500000, 25, false, { 0, 0, false, false }, 2, 1, { 103, 25, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 8, 128, 256 },
    { 129, 1500000, 25, false, { 0, 0, false, false }, 2, 1, { 104, 25, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 4, 128, 256 },
    { 256, 1500000, 51, false, { 0, 0, false, false }, 2, 1, { 205, 51, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 4, 128, 256 },
    { 257, 1500000, 51, false, { 0, 0, false, false }, 2, 1, { 206, 51, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 2, 128, 256 },
    { 384, 1500000, 76, false, { 0, 0, false, false }, 2, 1, { 308, 76, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 2, 128, 256 },
    { 385, 1500000, 77, false, { 0, 0, false, false }, 2, 1, { 308, 77, 0, 0 }, { 4, 4, 0, 0 }, true, 512, 2, 128, 256 },
    { 640, 1500000, 128, false, { 0, 0, false, false }, 3, 2, { 170, 342, 128, 0 }, { 4, 4, 4, 0 }, true, 512, 2, 128, 256 },
    { 641, 1500000, 128, false, { 0, 0, false, false }, 3, 2, { 171, 342, 128, 0 }, { 4, 4, 4, 0 }, true, 256, 1, 128, 256 },
    { 800, 1500000, 160, false, { 0, 0, false, false }, 4, 3, { 106, 214, 320, 160 }, { 4, 4, 4, 4 }, true, 256, 1, 128, 256 },
    { 801, 1500000, 160, false, { 0, 0, false, false }, 4, 3, { 106, 214, 321, 160 }, { 4, 4, 4, 4 }, true, 256, 1, 128, 256 },
    { 1280, 1500000, 256, false, { 0, 0, false, false }, 4, 3, { 170, 342, 512, 256 }, { 4, 4, 4, 4 }, true, 256, 1, 128, 256 },
    { 1281, 1500000, 256, false, { 0, 0, false, false }, 4, 3, { 170, 342, 513, 256 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 0, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 1, 1500000, 0, true, { 0, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 63, 1500000, 12, true, { 0, 0, false, false }, 1, -1, { 63, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 64, 1500000, 12, true, { 0, 0, false, false }, 1, -1, { 64, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 32, 256 },
    { 128, 1500000, 25, true, { 0, 0, false, false }, 2, 1, { 103, 25, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 8, 32, 256 },
    { 129, 1500000, 25, true, { 0, 0, false, false }, 2, 1, { 104, 25, 0, 0 }, { 4, 4, 0, 0 }, true, 512, 4, 32, 256 },
    { 256, 1500000, 51, true, { 0, 0, false, false }, 2, 1, { 205, 51, 0, 0 }, { 4, 4, 0, 0 }, true, 512, 4, 32, 1024 },
    { 257, 1500000, 51, true, { 0, 0, false, false }, 2, 1, { 206, 51, 0, 0 }, { 4, 4, 0, 0 }, true, 256, 2, 32, 1024 },
    { 384, 1500000, 76, true, { 0, 0, false, false }, 2, 1, { 308, 76, 0, 0 }, { 4, 4, 0, 0 }, true, 256, 2, 32, 1024 },
    { 385, 1500000, 77, true, { 0, 0, false, false }, 2, 1, { 308, 77, 0, 0 }, { 4, 4, 0, 0 }, true, 256, 2, 32, 1024 },
    { 640, 1500000, 128, true, { 0, 0, false, false }, 3, 2, { 170, 342, 128, 0 }, { 4, 4, 4, 0 }, true, 256, 2, 32, 1024 },
    { 641, 1500000, 128, true, { 0, 0, false, false }, 3, 2, { 171, 342, 128, 0 }, { 4, 4, 4, 0 }, true, 256, 1, 32, 1024 },
    { 800, 1500000, 160, true, { 0, 0, false, false }, 4, 3, { 106, 214, 320, 160 }, { 4, 4, 4, 4 }, true, 256, 1, 32, 1024 },
    { 801, 1500000, 160, true, { 0, 0, false, false }, 4, 3, { 106, 214, 321, 160 }, { 1, 1, 1, 4 }, true, 256, 1, 32, 1024 },
    { 1280, 1500000, 256, true, { 0, 0, false, false }, 4, 3, { 170, 342, 512, 256 }, { 1, 1, 1, 4 }, true, 256, 1, 32, 1024 },
    { 1281, 1500000, 256, true, { 0, 0, false, false }, 4, 3, { 170, 342, 513, 256 }, { 1, 1, 1, 4 }, false, 256, 1, 32, 1024 },
    { 2560, 1500000, 512, true, { 0, 0, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 32, 1024 },
    /* the edges of the expensive rule: 15 / 16 blocks, 35 % of the batch, 45 % of the largest cost */
    { 64, 1500000, 15, false, { 0, 0, false, false }, 1, -1, { 64, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 64, 1500000, 16, false, { 0, 0, false, false }, 2, 1, { 48, 16, 0, 0 }, { 8, 8, 0, 0 }, true, 1024, 8, 128, 256 },
    { 45, 1500000, 16, false, { 0, 0, false, false }, 1, -1, { 45, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 46, 1500000, 16, false, { 0, 0, false, false }, 1, -1, { 46, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 100, 1500000, 35, false, { 0, 0, false, false }, 2, 1, { 65, 35, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 8, 128, 256 },
    { 100, 1500000, 36, false, { 0, 0, false, false }, 1, -1, { 100, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 8, 128, 256 },
    { 400, 1500000, 140, false, { 0, 0, false, false }, 2, 1, { 260, 140, 0, 0 }, { 4, 4, 0, 0 }, true, 512, 2, 128, 256 },
    { 400, 1500000, 141, false, { 0, 0, false, false }, 1, -1, { 400, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 200, 2700000, 40, false, { 0, 0, false, false }, 2, 1, { 160, 40, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 4, 128, 256 },
    { 200, 2700001, 40, false, { 0, 0, false, false }, 1, -1, { 200, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 4, 128, 256 },
    /* the chunk count by 5.5 ns per bit against 0.04 ms per block */
    { 1000, 6000000, 0, false, { 0, 0, false, false }, 1, -1, { 1000, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 256, 1, 128, 256 },
    { 1700, 6000000, 0, false, { 0, 0, false, false }, 2, -1, { 566, 1134, 0, 0 }, { 1, 1, 0, 0 }, false, 256, 1, 128, 256 },
    { 2000, 6000000, 0, false, { 0, 0, false, false }, 2, -1, { 666, 1334, 0, 0 }, { 1, 1, 0, 0 }, false, 256, 1, 128, 256 },
    /* the overrides of the tests (scan waves, table-build slices, narrow k_mtf) and MI355X_BZ2_NO_SPLIT */
    { 1, 1500000, 0, false, { 1, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 1, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 1, 1500000, 0, false, { 4, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 4, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 1, 1500000, 0, false, { 8, 0, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 1, 1500000, 0, false, { 0, 1, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 1, 128, 256 },
    { 1, 1500000, 0, false, { 0, 2, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 2, 128, 256 },
    { 1, 1500000, 0, false, { 0, 4, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 4, 128, 256 },
    { 1, 1500000, 0, false, { 0, 16, false, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 1, 1500000, 0, false, { 0, 0, true, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 256, 8, 128, 256 },
    { 1, 1500000, 0, true, { 0, 0, true, false }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 256, 8, 32, 256 },
    { 1, 1500000, 0, false, { 0, 0, false, true }, 1, -1, { 1, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 1024, 8, 128, 256 },
    { 300, 1500000, 60, false, { 1, 0, false, false }, 2, 1, { 240, 60, 0, 0 }, { 1, 1, 0, 0 }, true, 512, 2, 128, 256 },
    { 300, 1500000, 60, false, { 4, 0, false, false }, 2, 1, { 240, 60, 0, 0 }, { 4, 4, 0, 0 }, true, 512, 2, 128, 256 },
    { 300, 1500000, 60, false, { 8, 0, false, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 2, 128, 256 },
    { 300, 1500000, 60, false, { 0, 1, false, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 1, 128, 256 },
    { 300, 1500000, 60, false, { 0, 2, false, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 2, 128, 256 },
    { 300, 1500000, 60, false, { 0, 4, false, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 4, 128, 256 },
    { 300, 1500000, 60, false, { 0, 16, false, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 512, 8, 128, 256 },
    { 300, 1500000, 60, false, { 0, 0, true, false }, 2, 1, { 240, 60, 0, 0 }, { 8, 8, 0, 0 }, true, 256, 2, 128, 256 },
    { 300, 1500000, 60, true, { 0, 0, true, false }, 2, 1, { 240, 60, 0, 0 }, { 4, 4, 0, 0 }, true, 256, 2, 32, 1024 },
    { 300, 1500000, 60, false, { 0, 0, false, true }, 1, -1, { 300, 0, 0, 0 }, { 8, 0, 0, 0 }, true, 512, 2, 128, 256 },
    { 2560, 1500000, 512, false, { 1, 0, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 1 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 4, 0, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 4, 4, 4, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 8, 0, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 8, 8, 8, 8 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 1, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 2, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 4, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 16, false, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, false, { 0, 0, true, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 128, 256 },
    { 2560, 1500000, 512, true, { 0, 0, true, false }, 4, 3, { 341, 683, 1024, 512 }, { 1, 1, 1, 4 }, false, 256, 1, 32, 1024 },
    { 2560, 1500000, 512, false, { 0, 0, false, true }, 1, -1, { 2560, 0, 0, 0 }, { 1, 0, 0, 0 }, false, 256, 1, 128, 256 },
};

void
check( const Case& c )
{
    uint64_t inSize = 0;
    const std::vector<uint64_t> offsets = layout( c, &inSize );
    const BatchPlan p = planBatch( offsets.data(), c.n, inSize, c.crowd, c.knobs );
    CHECK( p.groups == c.groups );
    CHECK( p.expensive == c.expensive );
    for ( int g = 0; g < MAX_GROUPS; ++g ) {
        CHECK( p.count[g] == c.count[g] );
        CHECK( g >= p.groups || p.scanWaves[g] == c.scanWaves[g] );
    }
    CHECK( p.mtfSide == c.mtfSide );
    CHECK( p.mtfSmallLanes == c.mtfSmallLanes );
    CHECK( p.bwtSlices == c.bwtSlices );
    CHECK( p.walkWgsPerXcd == c.walkWgsPerXcd );
    CHECK( p.walkChunk == c.walkChunk );

    /* the groups tile the slots in order */
    uint32_t next = 0;
    for ( int g = 0; g < p.groups; ++g ) {
        CHECK( p.first[g] == next );
        next += p.count[g];
    }
    CHECK( next == c.n );
    /* slotOf is a permutation, and the offsets by slot follow it */
    CHECK( p.slotOf.size() == c.n && p.offsets.size() == c.n && p.order.size() == c.n );
    std::vector<int> seen( c.n, 0 );
    for ( uint32_t i = 0; i < c.n && i < p.slotOf.size(); ++i ) {
        CHECK( p.slotOf[i] < c.n );
        if ( p.slotOf[i] >= c.n ) continue;
        ++seen[p.slotOf[i]];
        CHECK( p.offsets[p.slotOf[i]] == offsets[i] );
    }
    for ( uint32_t s = 0; s < c.n; ++s ) CHECK( seen[s] == 1 );
    /* inside each group: the group-relative slots, descending */
    for ( int g = 0; g < p.groups && next == c.n; ++g ) {
        for ( uint32_t k = 0; k < p.count[g]; ++k ) CHECK( p.order[p.first[g] + k] == p.count[g] - 1 - k );
    }
}
}  // namespace

int
main()
{
    for ( const Case& c : CASES ) check( c );

    /* two anchors, spelled out */
    {
        const Case c{ 2560, 6000000, 0, true, {}, 0, 0, {}, {}, false, 0, 0, 0, 0 };
        uint64_t inSize = 0;
        const auto offsets = layout( c, &inSize );
        const BatchPlan p = planBatch( offsets.data(), c.n, inSize, /* crowd */ true, {} );
        CHECK( p.expensive == -1 && p.groups == 3 );
        CHECK( p.count[0] == 426 && p.count[1] == 854 && p.count[2] == 1280 );
        CHECK( p.scanWaves[0] == 1 && p.scanWaves[1] == 1 && p.scanWaves[2] == 1 );
        CHECK( !p.mtfSide && p.bwtSlices == 1 && p.walkWgsPerXcd == 32 && p.walkChunk == 1024 );
    }
    {
        const Case c{ 1, 6000000, 0, false, {}, 0, 0, {}, {}, false, 0, 0, 0, 0 };
        uint64_t inSize = 0;
        const auto offsets = layout( c, &inSize );
        const BatchPlan p = planBatch( offsets.data(), c.n, inSize, /* crowd */ false, {} );
        CHECK( p.groups == 1 && p.scanWaves[0] == 8 );
        CHECK( p.mtfSide && p.mtfSmallLanes == 1024 && p.bwtSlices == 8 && p.walkWgsPerXcd == 128 && p.walkChunk == 256 );
    }
    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "plan ok: %zu cases\n", sizeof( CASES ) / sizeof( CASES[0] ) );
    return 0;
}
