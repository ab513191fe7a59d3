/**
 * bz2_distinct.hip -- the distinct values among the line hashes of a file (mi355x_bz2_reader_distinct_lines), and the
 * device memory the reader keeps those hashes in.
 *
 *   k_iota            numbers[i] = i
 *   rocPRIM           a stable radix sort of ( hash, line number ) over the 61 bits of a hash: equal hashes stay in line
 *                     order, so the first element of a run is the line's first occurrence
 *   k_flag_runs       flags[i] = i == 0 || hash[i] != hash[i - 1], and the number of flags (one atomic per workgroup)
 *   rocPRIM           with the numbers wanted: select the flagged line numbers, sort them ascending
 *
 * and the groups of the lines of a range by the key of a field (mi355x_bz2_reader_field_groups), with the same sort:
 *
 *   rocPRIM           the stable sort of ( key, line ) and k_flag_runs as above; select the flagged POSITIONS: run starts
 *   k_group_runs      per run: its length (to the next run's start), its first line (stability: the run's first element),
 *                     that line's field span gathered from the span column; the last run's length goes aside if its key
 *                     is the one that stands for a missing field, the largest 61-bit value
 *   rocPRIM           sort ( first line, run ) ascending
 *   k_group_order     the groups in that order, 32 bytes each, for the one D2H
 *
 * and those groups with the numbers of a second field summed per group (mi355x_bz2_reader_field_sums):
 *
 *   rocPRIM           the stable sort of ( key, line ) and k_flag_runs as above, for the number of runs; then ONE
 *                     reduce-by-key over the sorted line numbers, each
 *                     read as the SumPart of its line's value: a 128-bit sum ( uint64 lo, int64 hi, with carry ), min, max,
 *                     the count of numbers, the count of lines and the least line.  Its cost does not depend on the
 *                     lengths of the runs: one key shared by every line costs what all-distinct keys cost
 *   k_sum_runs        per run: the group from its SumPart and its first line's key span; the last run's length goes
 *                     aside if its key stands for a missing field
 *   rocPRIM           sort ( first line, run ) ascending
 *   k_sum_order       the groups in that order, 72 bytes each, for the one D2H
 *
 * and the numbers of the lines that a predicate selects (mi355x_bz2_reader_field_matches, _field_in_range):
 *
 *   rocPRIM           ONE select over a counting iterator, the predicate reading the line's flag word (k_field_match wrote
 *                     it) or its field-number word against lo and hi, inverted or not: the selected numbers ascend, their
 *                     count takes 8 bytes to the host
 *   k_number_lines    + the number of the range's first line, over the numbers that are kept (the first `limit`)
 *
 * The null stream and buffers of the call's own: it comes when the reader's launches are through.  Every buffer is
 * allocated before the pass that fills it, so that a failed allocation loses no result.
 */
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "bz2_ctx.hpp"

namespace
{
constexpr uint32_t DISTINCT_THREADS = 256;

__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_iota( uint64_t* __restrict__ numbers, uint64_t n )
{
    const uint64_t i = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( i < n ) numbers[i] = i;
}

__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_flag_runs( const uint64_t* __restrict__ sorted, uint64_t n, uint8_t* __restrict__ flags, unsigned long long* __restrict__ count )
{
    __shared__ uint32_t inBlock;
    if ( threadIdx.x == 0 ) inBlock = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( i < n ) {
        const bool first = i == 0 || sorted[i] != sorted[i - 1];
        flags[i] = first ? 1 : 0;
        if ( first ) atomicAdd( &inBlock, 1u );
    }
    __syncthreads();
    if ( threadIdx.x == 0 && inBlock != 0 ) atomicAdd( count, (unsigned long long)inBlock );
}

/** One lane per run of equal keys in the sorted column; runStarts ascend. */
__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_group_runs( const uint64_t* __restrict__ runStarts, uint64_t nRuns, uint64_t n, const uint64_t* __restrict__ sortedKeys,
              const uint64_t* __restrict__ sortedNumbers, const uint64_t* __restrict__ starts, const int64_t* __restrict__ sizes,
              uint64_t missing, mi355x::FieldGroup* __restrict__ groups, uint64_t* __restrict__ firstLines,
              uint64_t* __restrict__ runs, unsigned long long* __restrict__ nMissing )
{
    const uint64_t r = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( r >= nRuns ) return;
    const uint64_t begin = runStarts[r], end = r + 1 < nRuns ? runStarts[r + 1] : n;
    const uint64_t line = sortedNumbers[begin];
    groups[r] = { line, end - begin, starts[line], sizes[line] };
    firstLines[r] = line;
    runs[r] = r;
    /* the keys ascend and `missing` is the largest there is */
    if ( r + 1 == nRuns && sortedKeys[begin] == missing ) *nMissing = end - begin;
}

__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_group_order( const mi355x::FieldGroup* __restrict__ groups, const uint64_t* __restrict__ order, uint64_t nGroups,
               mi355x::FieldGroup* __restrict__ ordered )
{
    const uint64_t i = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( i < nGroups ) ordered[i] = groups[order[i]];
}

/** What reduce-by-key carries per run of equal keys in groupSums: the exact sum of the numbers as 128 bits, their least,
 * their largest and their count, the count of lines and the first line. */
struct SumPart
{
    uint64_t lo;
    int64_t hi, min, max;
    uint64_t numbers, count, line;
};

constexpr int64_t SUM_NOT_A_NUMBER = bz2gpu::FIELD_NOT_A_NUMBER, SUM_MISSING = bz2gpu::FIELD_NUMBER_MISSING;

/** The SumPart of one sorted element: line number -> that line's value. */
struct SumOfLine
{
    const int64_t* values;

    __device__ SumPart
    operator()( uint64_t line ) const
    {
        const int64_t value = values[line];
        if ( value == SUM_NOT_A_NUMBER || value == SUM_MISSING ) return { 0, 0, INT64_MAX, INT64_MIN, 0, 1, line };
        return { (uint64_t)value, value < 0 ? -1 : 0, value, value, 1, 1, line };
    }
};

/** Two SumParts as one: associative and commutative. */
struct SumJoin
{
    __device__ SumPart
    operator()( const SumPart& a, const SumPart& b ) const
    {
        const uint64_t lo = a.lo + b.lo;
        return { lo, a.hi + b.hi + ( lo < a.lo ? 1 : 0 ), a.min < b.min ? a.min : b.min, a.max > b.max ? a.max : b.max,
                 a.numbers + b.numbers, a.count + b.count, a.line < b.line ? a.line : b.line };
    }
};

/** One lane per run of equal keys: keys[r] ascend and parts[r] is the run's reduction. */
__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_sum_runs( const uint64_t* __restrict__ keys, const SumPart* __restrict__ parts, uint64_t nRuns, const uint64_t* __restrict__ starts,
            const int64_t* __restrict__ sizes, uint64_t missing, mi355x::FieldSumGroup* __restrict__ groups,
            uint64_t* __restrict__ firstLines, uint64_t* __restrict__ runs, unsigned long long* __restrict__ nMissing )
{
    const uint64_t r = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( r >= nRuns ) return;
    const SumPart part = parts[r];
    const bool none = part.numbers == 0;
    groups[r] = { part.line, part.count, starts[part.line], sizes[part.line], part.numbers, part.lo, part.hi,
                  none ? SUM_NOT_A_NUMBER : part.min, none ? SUM_NOT_A_NUMBER : part.max };
    firstLines[r] = part.line;
    runs[r] = r;
    /* the keys ascend and `missing` is the largest there is */
    if ( r + 1 == nRuns && keys[r] == missing ) *nMissing = part.count;
}

__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_sum_order( const mi355x::FieldSumGroup* __restrict__ groups, const uint64_t* __restrict__ order, uint64_t nGroups,
             mi355x::FieldSumGroup* __restrict__ ordered )
{
    const uint64_t i = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( i < nGroups ) ordered[i] = groups[order[i]];
}

/** Device allocations of one call, freed when it returns. */
struct Buffers
{
    std::vector<void*> pointers;
    const char* who{ "distinct_lines" };

    ~Buffers()
    {
        for ( auto* const pointer : pointers ) (void)hipFree( pointer );
    }
    template<typename T>
    bool
    get( T** pointer, uint64_t bytes, const char* what, std::string* error )
    {
        void* raw = nullptr;
        const hipError_t err = hipMalloc( &raw, bytes > 0 ? bytes : 1 );
        if ( err != hipSuccess ) {
            (void)hipGetLastError();
            *error = std::string( who ) + ": no device memory for " + what + " (" + std::to_string( bytes ) + " bytes): "
                     + hipGetErrorString( err );
            return false;
        }
        pointers.push_back( raw );
        *pointer = static_cast<T*>( raw );
        return true;
    }
};

bool
tried( hipError_t err, const char* what, std::string* error )
{
    if ( err == hipSuccess ) return true;
    *error = std::string( what ) + ": " + hipGetErrorString( err );
    return false;
}

#define DISTINCT_TRY( expr ) \
    do { if ( !tried( ( expr ), #expr, error ) ) return false; } while ( 0 )
}  // namespace

void*
mi355x::deviceAllocate( int device, uint64_t bytes, std::string* error )
{
    void* pointer = nullptr;
    hipError_t err = device >= 0 ? hipSetDevice( device ) : hipSuccess;
    if ( err == hipSuccess ) err = hipMalloc( &pointer, bytes > 0 ? bytes : 1 );
    if ( err != hipSuccess ) {
        (void)hipGetLastError();
        *error = "no device memory for " + std::to_string( bytes ) + " bytes of line hashes: " + hipGetErrorString( err );
        return nullptr;
    }
    return pointer;
}

void
mi355x::deviceRelease( void* pointer )
{
    if ( pointer != nullptr ) (void)hipFree( pointer );
}

bool
mi355x::deviceToHost( int device, void* dst, const void* src, uint64_t bytes, bool dstIsDevice, std::string* error )
{
    if ( bytes == 0 ) return true;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    DISTINCT_TRY( hipMemcpy( dst, src, bytes, dstIsDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost ) );
    return true;
}

bool
mi355x::hostToDevice( int device, void* dst, const void* src, uint64_t bytes, std::string* error )
{
    if ( bytes == 0 ) return true;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    DISTINCT_TRY( hipMemcpy( dst, src, bytes, hipMemcpyHostToDevice ) );
    return true;
}

namespace
{
/** Item i of columnOffsets' scan: the bytes of line i's field, and nothing for the one item behind the lines. */
struct BytesOfLine
{
    const int64_t* sizes;
    uint64_t n;

    __device__ uint64_t
    operator()( uint64_t i ) const
    {
        const int64_t size = i < n ? sizes[i] : 0;
        return size > 0 ? (uint64_t)size : 0;
    }
};
}  // namespace

bool
mi355x::columnOffsets( int device, const int64_t* dSizes, uint64_t n, uint64_t* dOffsets, uint64_t* total, std::string* error )
{
    *total = 0;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    const hipStream_t stream = nullptr;
    /* n + 1 items, the last one 0: the exclusive scan's last value is the total */
    const auto bytes = rocprim::make_transform_iterator( rocprim::make_counting_iterator( uint64_t( 0 ) ), BytesOfLine{ dSizes, n } );
    Buffers buffers;
    buffers.who = "field_columns";
    void* dTemp = nullptr;
    size_t tempBytes = 0;
    DISTINCT_TRY( rocprim::exclusive_scan( nullptr, tempBytes, bytes, dOffsets, uint64_t( 0 ), (size_t)n + 1, rocprim::plus<uint64_t>(), stream ) );
    if ( !buffers.get( &dTemp, tempBytes, "the scan", error ) ) return false;
    DISTINCT_TRY( rocprim::exclusive_scan( dTemp, tempBytes, bytes, dOffsets, uint64_t( 0 ), (size_t)n + 1, rocprim::plus<uint64_t>(), stream ) );
    DISTINCT_TRY( hipMemcpyAsync( total, dOffsets + n, sizeof( uint64_t ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    return true;
}

bool
mi355x::distinctHashes( int device, const uint64_t* dHashes, uint64_t n, uint64_t* nDistinct, std::vector<uint64_t>* numbers,
                        std::string* error )
{
    *nDistinct = 0;
    if ( numbers != nullptr ) numbers->clear();
    if ( n == 0 ) return true;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    const hipStream_t stream = nullptr;
    const uint32_t blocks = (uint32_t)( ( n + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS );
    if ( (uint64_t)blocks * DISTINCT_THREADS < n ) {
        *error = "distinct_lines: too many lines";
        return false;
    }

    Buffers buffers;
    uint64_t *dNumbers = nullptr, *dSortedHashes = nullptr, *dSortedNumbers = nullptr;
    uint8_t* dFlags = nullptr;
    unsigned long long* dCount = nullptr;
    void* dTemp = nullptr;
    size_t sortBytes = 0;
    DISTINCT_TRY( rocprim::radix_sort_pairs( nullptr, sortBytes, dHashes, dSortedHashes, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );
    if ( !buffers.get( &dNumbers, n * 8, "the line numbers", error ) || !buffers.get( &dSortedHashes, n * 8, "the sorted hashes", error )
         || !buffers.get( &dSortedNumbers, n * 8, "the sorted line numbers", error ) || !buffers.get( &dFlags, n, "the flags", error )
         || !buffers.get( &dCount, 2 * sizeof( unsigned long long ), "the count", error )
         || !buffers.get( &dTemp, sortBytes, "the sort", error ) ) {
        return false;
    }
    DISTINCT_TRY( hipMemsetAsync( dCount, 0, 2 * sizeof( unsigned long long ), stream ) );
    hipLaunchKernelGGL( k_iota, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dNumbers, n );
    DISTINCT_TRY( hipGetLastError() );
    DISTINCT_TRY( rocprim::radix_sort_pairs( dTemp, sortBytes, dHashes, dSortedHashes, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );
    hipLaunchKernelGGL( k_flag_runs, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dSortedHashes, n, dFlags, dCount );
    DISTINCT_TRY( hipGetLastError() );
    unsigned long long count = 0;
    DISTINCT_TRY( hipMemcpyAsync( &count, dCount, sizeof( count ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    *nDistinct = count;
    if ( numbers == nullptr ) return true;

    /* the selected numbers go where the unsorted ones were, their sorted form where the sorted hashes were */
    try {
        numbers->resize( (size_t)count );
    } catch ( const std::exception& ) {
        *error = "distinct_lines: no host memory for " + std::to_string( count ) + " line numbers";
        return false;
    }
    uint64_t* const dSelected = dNumbers;
    uint64_t* const dAscending = dSortedHashes;
    size_t selectBytes = 0, secondSortBytes = 0;
    DISTINCT_TRY( rocprim::select( nullptr, selectBytes, dSortedNumbers, dFlags, dSelected, dCount + 1, (size_t)n, stream ) );
    DISTINCT_TRY( rocprim::radix_sort_keys( nullptr, secondSortBytes, dSelected, dAscending, (size_t)count, 0, 64, stream ) );
    void* dTemp2 = dTemp;
    if ( std::max( selectBytes, secondSortBytes ) > sortBytes
         && !buffers.get( &dTemp2, std::max( selectBytes, secondSortBytes ), "the selection", error ) ) {
        return false;
    }
    DISTINCT_TRY( rocprim::select( dTemp2, selectBytes, dSortedNumbers, dFlags, dSelected, dCount + 1, (size_t)n, stream ) );
    DISTINCT_TRY( rocprim::radix_sort_keys( dTemp2, secondSortBytes, dSelected, dAscending, (size_t)count, 0, 64, stream ) );
    DISTINCT_TRY( hipMemcpyAsync( numbers->data(), dAscending, count * 8, hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    return true;
}

bool
mi355x::groupHashes( int device, const uint64_t* dKeys, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n, uint64_t missing,
                     std::vector<FieldGroup>* groups, uint64_t* nMissing, std::string* error )
{
    static_assert( sizeof( FieldGroup ) == 32, "32 bytes per group come to the host" );
    groups->clear();
    *nMissing = 0;
    if ( n == 0 ) return true;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    const hipStream_t stream = nullptr;
    const uint32_t blocks = (uint32_t)( ( n + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS );
    if ( (uint64_t)blocks * DISTINCT_THREADS < n ) {
        *error = "field_groups: too many lines";
        return false;
    }

    Buffers buffers;
    buffers.who = "field_groups";
    uint64_t *dNumbers = nullptr, *dSortedKeys = nullptr, *dSortedNumbers = nullptr;
    uint8_t* dFlags = nullptr;
    unsigned long long* dCount = nullptr;     /* runs, selected, lines with a missing field */
    void* dTemp = nullptr;
    size_t sortBytes = 0, selectBytes = 0;
    const rocprim::counting_iterator<uint64_t> positions( 0 );
    DISTINCT_TRY( rocprim::radix_sort_pairs( nullptr, sortBytes, dKeys, dSortedKeys, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );
    DISTINCT_TRY( rocprim::select( nullptr, selectBytes, positions, dFlags, dNumbers, dCount + 1, (size_t)n, stream ) );
    if ( !buffers.get( &dNumbers, n * 8, "the line numbers", error ) || !buffers.get( &dSortedKeys, n * 8, "the sorted keys", error )
         || !buffers.get( &dSortedNumbers, n * 8, "the sorted line numbers", error ) || !buffers.get( &dFlags, n, "the flags", error )
         || !buffers.get( &dCount, 3 * sizeof( unsigned long long ), "the counts", error )
         || !buffers.get( &dTemp, std::max( sortBytes, selectBytes ), "the sort", error ) ) {
        return false;
    }
    DISTINCT_TRY( hipMemsetAsync( dCount, 0, 3 * sizeof( unsigned long long ), stream ) );
    hipLaunchKernelGGL( k_iota, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dNumbers, n );
    DISTINCT_TRY( hipGetLastError() );
    DISTINCT_TRY( rocprim::radix_sort_pairs( dTemp, sortBytes, dKeys, dSortedKeys, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );
    hipLaunchKernelGGL( k_flag_runs, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dSortedKeys, n, dFlags, dCount );
    DISTINCT_TRY( hipGetLastError() );
    /* the run starts go where the unsorted numbers were */
    uint64_t* const dRunStarts = dNumbers;
    DISTINCT_TRY( rocprim::select( dTemp, selectBytes, positions, dFlags, dRunStarts, dCount + 1, (size_t)n, stream ) );
    unsigned long long nRuns = 0;
    DISTINCT_TRY( hipMemcpyAsync( &nRuns, dCount, sizeof( nRuns ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );

    FieldGroup *dGroups = nullptr, *dOrdered = nullptr;
    uint64_t *dFirstLines = nullptr, *dRuns = nullptr, *dSortedLines = nullptr, *dOrder = nullptr;
    void* dTemp2 = nullptr;
    size_t orderBytes = 0;
    DISTINCT_TRY( rocprim::radix_sort_pairs( nullptr, orderBytes, dFirstLines, dSortedLines, dRuns, dOrder, (size_t)nRuns, 0, 64, stream ) );
    if ( !buffers.get( &dGroups, nRuns * sizeof( FieldGroup ), "the groups", error )
         || !buffers.get( &dOrdered, nRuns * sizeof( FieldGroup ), "the ordered groups", error )
         || !buffers.get( &dFirstLines, nRuns * 8, "the first lines", error ) || !buffers.get( &dRuns, nRuns * 8, "the runs", error )
         || !buffers.get( &dSortedLines, nRuns * 8, "the sorted first lines", error )
         || !buffers.get( &dOrder, nRuns * 8, "the order", error ) || !buffers.get( &dTemp2, orderBytes, "the second sort", error ) ) {
        return false;
    }
    const uint32_t runBlocks = (uint32_t)( ( nRuns + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS );
    hipLaunchKernelGGL( k_group_runs, dim3( runBlocks ), dim3( DISTINCT_THREADS ), 0, stream, dRunStarts, (uint64_t)nRuns, n, dSortedKeys,
                        dSortedNumbers, dStarts, dSizes, missing, dGroups, dFirstLines, dRuns, dCount + 2 );
    DISTINCT_TRY( hipGetLastError() );
    unsigned long long missingLines = 0;
    DISTINCT_TRY( hipMemcpyAsync( &missingLines, dCount + 2, sizeof( missingLines ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    *nMissing = missingLines;
    /* the run of the missing key is the last one: the groups are the runs in front of it */
    const uint64_t nGroups = nRuns - ( missingLines != 0 ? 1 : 0 );
    if ( nGroups == 0 ) return true;
    try {
        groups->resize( (size_t)nGroups );
    } catch ( const std::exception& ) {
        *error = "field_groups: no host memory for " + std::to_string( nGroups ) + " groups";
        return false;
    }
    DISTINCT_TRY( rocprim::radix_sort_pairs( dTemp2, orderBytes, dFirstLines, dSortedLines, dRuns, dOrder, (size_t)nGroups, 0, 64, stream ) );
    hipLaunchKernelGGL( k_group_order, dim3( (uint32_t)( ( nGroups + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS ) ), dim3( DISTINCT_THREADS ),
                        0, stream, dGroups, dOrder, nGroups, dOrdered );
    DISTINCT_TRY( hipGetLastError() );
    DISTINCT_TRY( hipMemcpyAsync( groups->data(), dOrdered, nGroups * sizeof( FieldGroup ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    return true;
}

bool
mi355x::groupSums( int device, const uint64_t* dKeys, const uint64_t* dStarts, const int64_t* dSizes, const int64_t* dValues, uint64_t n,
                   uint64_t missing, std::vector<FieldSumGroup>* groups, uint64_t* nMissing, std::string* error )
{
    static_assert( sizeof( FieldSumGroup ) == 72, "72 bytes per group come to the host" );
    groups->clear();
    *nMissing = 0;
    if ( n == 0 ) return true;
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    const hipStream_t stream = nullptr;
    const uint32_t blocks = (uint32_t)( ( n + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS );
    if ( (uint64_t)blocks * DISTINCT_THREADS < n ) {
        *error = "field_sums: too many lines";
        return false;
    }

    Buffers buffers;
    buffers.who = "field_sums";
    uint64_t *dNumbers = nullptr, *dSortedKeys = nullptr, *dSortedNumbers = nullptr, *dRunKeys = nullptr;
    uint8_t* dFlags = nullptr;
    SumPart* dParts = nullptr;
    unsigned long long* dCount = nullptr;     /* runs, lines with a missing key field, the reduction's runs */
    void* dTemp = nullptr;
    size_t sortBytes = 0, reduceBytes = 0;
    DISTINCT_TRY( rocprim::radix_sort_pairs( nullptr, sortBytes, dKeys, dSortedKeys, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );
    if ( !buffers.get( &dNumbers, n * 8, "the line numbers", error ) || !buffers.get( &dSortedKeys, n * 8, "the sorted keys", error )
         || !buffers.get( &dSortedNumbers, n * 8, "the sorted line numbers", error ) || !buffers.get( &dFlags, n, "the flags", error )
         || !buffers.get( &dCount, 3 * sizeof( unsigned long long ), "the counts", error )
         || !buffers.get( &dTemp, sortBytes, "the sort", error ) ) {
        return false;
    }
    DISTINCT_TRY( hipMemsetAsync( dCount, 0, 3 * sizeof( unsigned long long ), stream ) );
    hipLaunchKernelGGL( k_iota, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dNumbers, n );
    DISTINCT_TRY( hipGetLastError() );
    DISTINCT_TRY( rocprim::radix_sort_pairs( dTemp, sortBytes, dKeys, dSortedKeys, dNumbers, dSortedNumbers, (size_t)n, 0, 61, stream ) );

    /* the runs are counted first, so that the reduction's output takes 56 bytes per run and not per line */
    hipLaunchKernelGGL( k_flag_runs, dim3( blocks ), dim3( DISTINCT_THREADS ), 0, stream, dSortedKeys, n, dFlags, dCount );
    DISTINCT_TRY( hipGetLastError() );
    unsigned long long nRuns = 0;
    DISTINCT_TRY( hipMemcpyAsync( &nRuns, dCount, sizeof( nRuns ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );

    /* one reduction over the values in sorted order, whatever the lengths of the runs; the runs' keys go where the
     * unsorted numbers were */
    dRunKeys = dNumbers;
    const auto values = rocprim::make_transform_iterator( dSortedNumbers, SumOfLine{ dValues } );
    DISTINCT_TRY( rocprim::reduce_by_key( nullptr, reduceBytes, dSortedKeys, values, (size_t)n, dRunKeys, dParts, dCount + 2, SumJoin{},
                                          rocprim::equal_to<uint64_t>{}, stream ) );
    void* dTempReduce = dTemp;
    if ( !buffers.get( &dParts, nRuns * sizeof( SumPart ), "the sums", error )
         || ( reduceBytes > sortBytes && !buffers.get( &dTempReduce, reduceBytes, "the reduction", error ) ) ) {
        return false;
    }
    DISTINCT_TRY( rocprim::reduce_by_key( dTempReduce, reduceBytes, dSortedKeys, values, (size_t)n, dRunKeys, dParts, dCount + 2, SumJoin{},
                                          rocprim::equal_to<uint64_t>{}, stream ) );

    FieldSumGroup *dGroups = nullptr, *dOrdered = nullptr;
    uint64_t *dFirstLines = nullptr, *dRuns = nullptr, *dSortedLines = nullptr, *dOrder = nullptr;
    void* dTemp2 = nullptr;
    size_t orderBytes = 0;
    DISTINCT_TRY( rocprim::radix_sort_pairs( nullptr, orderBytes, dFirstLines, dSortedLines, dRuns, dOrder, (size_t)nRuns, 0, 64, stream ) );
    if ( !buffers.get( &dGroups, nRuns * sizeof( FieldSumGroup ), "the groups", error )
         || !buffers.get( &dOrdered, nRuns * sizeof( FieldSumGroup ), "the ordered groups", error )
         || !buffers.get( &dFirstLines, nRuns * 8, "the first lines", error ) || !buffers.get( &dRuns, nRuns * 8, "the runs", error )
         || !buffers.get( &dSortedLines, nRuns * 8, "the sorted first lines", error )
         || !buffers.get( &dOrder, nRuns * 8, "the order", error ) || !buffers.get( &dTemp2, orderBytes, "the second sort", error ) ) {
        return false;
    }
    const uint32_t runBlocks = (uint32_t)( ( nRuns + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS );
    hipLaunchKernelGGL( k_sum_runs, dim3( runBlocks ), dim3( DISTINCT_THREADS ), 0, stream, dRunKeys, dParts, (uint64_t)nRuns, dStarts,
                        dSizes, missing, dGroups, dFirstLines, dRuns, dCount + 1 );
    DISTINCT_TRY( hipGetLastError() );
    unsigned long long missingLines = 0;
    DISTINCT_TRY( hipMemcpyAsync( &missingLines, dCount + 1, sizeof( missingLines ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    *nMissing = missingLines;
    /* the run of the missing key is the last one: the groups are the runs in front of it */
    const uint64_t nGroups = nRuns - ( missingLines != 0 ? 1 : 0 );
    if ( nGroups == 0 ) return true;
    try {
        groups->resize( (size_t)nGroups );
    } catch ( const std::exception& ) {
        *error = "field_sums: no host memory for " + std::to_string( nGroups ) + " groups";
        return false;
    }
    DISTINCT_TRY( rocprim::radix_sort_pairs( dTemp2, orderBytes, dFirstLines, dSortedLines, dRuns, dOrder, (size_t)nGroups, 0, 64, stream ) );
    hipLaunchKernelGGL( k_sum_order, dim3( (uint32_t)( ( nGroups + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS ) ), dim3( DISTINCT_THREADS ),
                        0, stream, dGroups, dOrder, nGroups, dOrdered );
    DISTINCT_TRY( hipGetLastError() );
    DISTINCT_TRY( hipMemcpyAsync( groups->data(), dOrdered, nGroups * sizeof( FieldSumGroup ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    return true;
}

namespace
{
/** Is line i selected: its flag word, or its field-number word against the range; inverted or not. */
struct LineSelected
{
    mi355x::LinePredicate by;

    __device__ bool
    operator()( uint64_t i ) const
    {
        const bool holds = by.dFlags != nullptr ? by.dFlags[i] != 0 : ( by.dNumbers[i] >= by.lo && by.dNumbers[i] <= by.hi );
        return holds != by.invert;
    }
};

/** numbers[i] += base for the first n. */
__global__ __launch_bounds__( DISTINCT_THREADS ) void
k_number_lines( uint64_t* __restrict__ numbers, uint64_t n, uint64_t base )
{
    const uint64_t i = (uint64_t)blockIdx.x * DISTINCT_THREADS + threadIdx.x;
    if ( i < n ) numbers[i] += base;
}
}  // namespace

bool
mi355x::selectLines( int device, const LinePredicate& predicate, uint64_t n, uint64_t base, uint64_t limit, uint64_t** selected,
                     uint64_t* nMatching, std::string* error )
{
    *selected = nullptr;
    *nMatching = 0;
    if ( n == 0 ) return true;
    if ( predicate.dFlags == nullptr && predicate.dNumbers == nullptr ) {
        *error = "select_lines: neither flags nor numbers";
        return false;
    }
    if ( device >= 0 ) DISTINCT_TRY( hipSetDevice( device ) );
    const hipStream_t stream = nullptr;
    Buffers buffers;
    buffers.who = "select_lines";
    uint64_t* dNumbers = nullptr;
    unsigned long long* dCount = nullptr;
    void* dTemp = nullptr;
    size_t selectBytes = 0;
    const rocprim::counting_iterator<uint64_t> lines( 0 );
    const LineSelected isSelected{ predicate };
    DISTINCT_TRY( rocprim::select( nullptr, selectBytes, lines, dNumbers, dCount, (size_t)n, isSelected, stream ) );
    if ( !buffers.get( &dNumbers, n * 8, "the line numbers", error ) || !buffers.get( &dCount, sizeof( unsigned long long ), "the count", error )
         || !buffers.get( &dTemp, selectBytes, "the selection", error ) ) {
        return false;
    }
    DISTINCT_TRY( hipMemsetAsync( dCount, 0, sizeof( unsigned long long ), stream ) );
    DISTINCT_TRY( rocprim::select( dTemp, selectBytes, lines, dNumbers, dCount, (size_t)n, isSelected, stream ) );
    unsigned long long count = 0;
    DISTINCT_TRY( hipMemcpyAsync( &count, dCount, sizeof( count ), hipMemcpyDeviceToHost, stream ) );
    DISTINCT_TRY( hipStreamSynchronize( stream ) );
    *nMatching = count;
    const uint64_t kept = std::min<uint64_t>( count, limit );
    if ( kept == 0 ) return true;
    if ( base != 0 ) {
        hipLaunchKernelGGL( k_number_lines, dim3( (uint32_t)( ( kept + DISTINCT_THREADS - 1 ) / DISTINCT_THREADS ) ), dim3( DISTINCT_THREADS ),
                            0, stream, dNumbers, kept, base );
        DISTINCT_TRY( hipGetLastError() );
    }
    auto* const held = static_cast<uint64_t*>( deviceAllocate( -1, kept * 8, error ) );
    if ( held == nullptr ) return false;
    if ( !tried( hipMemcpyAsync( held, dNumbers, kept * 8, hipMemcpyDeviceToDevice, stream ), "hipMemcpyAsync", error )
         || !tried( hipStreamSynchronize( stream ), "hipStreamSynchronize", error ) ) {
        deviceRelease( held );
        return false;
    }
    *selected = held;
    return true;
}
