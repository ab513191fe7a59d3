/**
 * bz2_buffers.cpp -- mi355x_bz2_decompress_buffers: many independent bzip2 buffers in shared GPU batches.
 *
 * Per upload window (bz2_buffers.hpp): the buffers are packed back to back and copied to the device, k_find_magic finds
 * the block magics, the candidates are decoded in launches of at most max_launch_blocks blocks -- each block bounded by
 * its own buffer's end (decodeBatchBegin's end_bytes) -- and after every launch the chain walk places the blocks that
 * lie on a buffer's chain into the context's result buffer with k_gather.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355x_bz2.h"
#include "bz2_buffers.hpp"
#include "bz2_ctx.hpp"

namespace
{
using namespace mi355x::buffers;

int
fail( mi355x_bz2_ctx* ctx, int status, const std::string& message )
{
    mi355x::setLastError( ctx, "decompress_buffers: " + message );
    return status;
}

/** Block-magic bit offsets of the resident window, ascending. */
int
scanWindow( mi355x_bz2_ctx* ctx, uint64_t windowBytes, std::vector<uint64_t>& matches )
{
    uint64_t found = 0;
    matches.resize( windowBytes / 2048 + 1024 );
    int rc = mi355x_bz2_find_magic_device( ctx, MI355X_BZ2_MAGIC_BLOCK, matches.data(), matches.size(), &found );
    if ( rc != MI355X_BZ2_OK ) return rc;
    if ( found > matches.size() ) {
        matches.resize( found );
        rc = mi355x_bz2_find_magic_device( ctx, MI355X_BZ2_MAGIC_BLOCK, matches.data(), matches.size(), &found );
        if ( rc != MI355X_BZ2_OK ) return rc;
    }
    matches.resize( found );
    return MI355X_BZ2_OK;
}
}  // namespace

extern "C" int
mi355x_bz2_decompress_buffers( mi355x_bz2_ctx* ctx, const uint8_t* const* buffers, const uint64_t* sizes, uint32_t n,
                               uint32_t maxLaunchBlocks, mi355x_bz2_buffer_result* results, uint64_t* totalDecoded )
{
    if ( ctx == nullptr || ( n > 0 && ( buffers == nullptr || sizes == nullptr || results == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    if ( maxLaunchBlocks > MI355X_BZ2_MAX_BATCH_BLOCKS ) {
        return fail( ctx, MI355X_BZ2_ERR_INVALID_ARGUMENT, "max_launch_blocks exceeds MI355X_BZ2_MAX_BATCH_BLOCKS" );
    }
    for ( uint32_t i = 0; i < n; ++i ) {
        if ( buffers[i] == nullptr && sizes[i] > 0 ) {
            return fail( ctx, MI355X_BZ2_ERR_INVALID_ARGUMENT, "buffer " + std::to_string( i ) + " is NULL" );
        }
    }
    if ( totalDecoded != nullptr ) *totalDecoded = 0;

    const auto windows = planWindows( sizes, n, WINDOW_BYTES );
    std::vector<uint8_t> packed;
    std::vector<uint64_t> matches;
    std::vector<mi355x_bz2_block_result> blockResults;
    std::vector<Record> records;
    uint64_t outputEnd = 0;    /* where the next buffer's bytes go */
    uint64_t written = 0;      /* bytes of the result buffer that hold gathered data */
    uint8_t* dResult = nullptr;
    int rc = MI355X_BZ2_OK;
    for ( const auto& window : windows ) {
        WindowPlan plan;
        if ( window.bytes == 0 ) {
            plan = planWindow( sizes + window.first, window.count, nullptr, 0, maxLaunchBlocks );
        } else {
            {
                /* the window is copied into the context's input buffer, which a smaller copy reuses */
                size_t freeBytes = 0, totalBytes = 0;
                if ( hipSetDevice( mi355x::deviceOf( ctx ) ) == hipSuccess
                     && hipMemGetInfo( &freeBytes, &totalBytes ) == hipSuccess
                     && window.bytes + ( 64u << 20 ) > freeBytes + mi355x::inputCapacity( ctx ) ) {
                    const std::string what =
                        window.count == 1
                            ? "buffer " + std::to_string( window.first ) + " (" + std::to_string( window.bytes )
                                  + " bytes) does not fit on the device: decode it with open(), which streams"
                            : "buffers " + std::to_string( window.first ) + " to "
                                  + std::to_string( window.first + window.count - 1 ) + " (one upload window of "
                                  + std::to_string( window.bytes ) + " bytes) do not fit beside what the device holds ("
                                  + std::to_string( freeBytes ) + " bytes free)";
                    return fail( ctx, MI355X_BZ2_ERR_INVALID_ARGUMENT, what );
                }
            }
            packed.resize( window.bytes );
            uint64_t at = 0;
            for ( uint32_t b = 0; b < window.count; ++b ) {
                const uint64_t size = sizes[window.first + b];
                if ( size > 0 ) std::memcpy( packed.data() + at, buffers[window.first + b], size );
                at += size;
            }
            rc = mi355x_bz2_set_input_host( ctx, packed.data(), packed.size() );
            if ( rc != MI355X_BZ2_OK ) return rc;
            rc = scanWindow( ctx, window.bytes, matches );
            if ( rc != MI355X_BZ2_OK ) return rc;
            plan = planWindow( sizes + window.first, window.count, matches.data(), matches.size(), maxLaunchBlocks );
        }

        ChainWalk walk( plan, buffers + window.first, outputEnd );
        for ( uint32_t k = 0; k < plan.launches.size(); ++k ) {
            const Launch& launch = plan.launches[k];
            blockResults.resize( launch.count );
            rc = mi355x::decodeBatchBegin( ctx, plan.bits.data() + launch.first, plan.endBytes.data() + launch.first,
                                           launch.count );
            if ( rc != MI355X_BZ2_OK ) return rc;
            uint64_t launchBytes = 0;
            rc = mi355x_bz2_decode_batch_end( ctx, blockResults.data(), &launchBytes );
            if ( rc != MI355X_BZ2_OK ) return rc;
            records.resize( launch.count );
            for ( uint32_t i = 0; i < launch.count; ++i ) {
                const auto& r = blockResults[i];
                records[i] = { r.encoded_size_bits, r.decoded_size, r.data_offset, r.computed_crc, r.status };
            }
            const auto pieces = walk.advance( k, records.data() );
            if ( pieces.empty() ) continue;
            uint64_t need = 0;
            for ( const auto& p : pieces ) need = std::max( need, p.dst + p.size );
            rc = mi355x::resultBuffer( ctx, need, written, &dResult );
            if ( rc != MI355X_BZ2_OK ) return rc;
            std::vector<mi355x_bz2_gather_piece> gather( pieces.size() );
            for ( size_t i = 0; i < pieces.size(); ++i ) gather[i] = { pieces[i].src, pieces[i].dst, pieces[i].size };
            rc = mi355x_bz2_gather_output( ctx, gather.data(), (uint32_t)gather.size(), dResult, 1 );
            if ( rc != MI355X_BZ2_OK ) return rc;
            written = std::max( written, need );
        }
        const auto& done = walk.finish();
        for ( uint32_t b = 0; b < window.count; ++b ) {
            const auto& d = done[b];
            auto& r = results[window.first + b];
            r.output_offset = d.outputOffset;
            r.decoded_size = d.decodedSize;
            r.error_offset_bits = d.errorOffsetBits;
            r.n_blocks = d.blocks;
            r.n_streams = d.streams;
            r.trailing_garbage = d.trailingGarbage ? 1 : 0;
            r.status = d.status;
        }
        outputEnd = walk.end();
    }
    rc = mi355x::resultBuffer( ctx, std::max<uint64_t>( outputEnd, 1 ), written, &dResult );
    if ( rc != MI355X_BZ2_OK ) return rc;
    rc = mi355x::publishResult( ctx, outputEnd );
    if ( rc != MI355X_BZ2_OK ) return rc;
    if ( totalDecoded != nullptr ) *totalDecoded = outputEnd;
    return MI355X_BZ2_OK;
}
