/**
 * bz2_reader.cpp -- reader + GPU batch scheduler behind C ABI section 3 of include/mi355x_bz2.h.
 *
 *   BatchScheduler  the role of rapidgzip::BlockFetcher + BZ2BlockFetcher    src/core/BlockFetcher.hpp:244-317, 446-559,
 *                                                                            src/indexed_bzip2/BZ2BlockFetcher.hpp:64-138
 *   StreamReader    the role of indexed_bzip2::ParallelBZ2Reader             src/indexed_bzip2/ParallelBZ2Reader.hpp:39-498
 *
 * What a caller can observe is the reference's: read / seek / tell / eof, the block-offset map with its end-of-stream
 * entries and end-of-file entry, "a block that cannot be decoded fails the read that needs it and no read before it",
 * trailing garbage is ignored with a warning, the stream CRC check of the serial reader.  The structure is this design's:
 * the unit of work is a RUN -- a batch of consecutive blocks decoded by one launch sequence into one page-locked host
 * buffer -- not a block.  The scheduler keeps runs (in flight and finished) by the number of their first block, decides
 * from the recent access pattern which RANGE of blocks to launch next, and hands out runs; the reader walks through a
 * run's blocks without further look-ups in caches, and bytes of consecutive blocks are consecutive in the run's buffer.
 */
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <iostream>
#include <list>
#include <memory>
#include <optional>
#include <queue>
#include <sstream>
#include <string>
#include <variant>

#include <hip/hip_runtime.h>

#include "../../include/mi355x_bz2.h"
#include "bz2_host.hpp"
#include "bz2_ctx.hpp"
#include "bz2_lines.hpp"
#include "bz2_linehash.hpp"
#include "bz2_fields.hpp"
#include "bz2_fieldcols.hpp"
#include "bz2_search.hpp"
#include "bz2_ranges.hpp"

namespace mi355x
{
struct Bz2Exception : public std::runtime_error
{
    Bz2Exception( int statusCode, const std::string& message ) :
        std::runtime_error( message ),
        status( statusCode )
    {}

    int status;
};

static Bz2Exception
error( int status, const std::string& detail = {} )
{
    std::string message = mi355x_bz2_status_string( status );
    if ( !detail.empty() ) {
        message += ": " + detail;
    }
    return Bz2Exception( status, message );
}

[[noreturn]] static void
fail( int status, const std::string& detail = {} )
{
    throw error( status, detail );
}

/** A failure of a call on a decoder context becomes an exception with the context's last error. */
static void
checkDevice( mi355x_bz2_ctx* ctx, int rc )
{
    if ( rc != MI355X_BZ2_OK ) fail( rc, mi355x_bz2_last_error( ctx ) );
}

/* ------------------------------------------------------------------------------------------------ compressed source */
class Source
{
public:
    static std::shared_ptr<Source>
    fromFd( int fd, bool closeFd )
    {
        struct stat st{};
        if ( fstat( fd, &st ) != 0 || !S_ISREG( st.st_mode ) ) {
            if ( closeFd ) ::close( fd );
            /* ParallelBZ2Reader.hpp:66-68 */
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "Parallel BZ2 Reader will not work on non-seekable input like stdin (yet)!" );
        }
        auto s = std::shared_ptr<Source>( new Source() );
        s->m_size = (uint64_t)st.st_size;
        if ( s->m_size > 0 ) {
            void* p = mmap( nullptr, s->m_size, PROT_READ, MAP_PRIVATE, fd, 0 );
            if ( p == MAP_FAILED ) {
                const int e = errno;
                if ( closeFd ) ::close( fd );
                fail( MI355X_BZ2_ERR_IO, std::string( "mmap: " ) + strerror( e ) );
            }
            s->m_map = p;
            s->m_bytes = static_cast<const uint8_t*>( p );
            (void)madvise( p, s->m_size, MADV_SEQUENTIAL );
        }
        if ( closeFd ) ::close( fd );
        return s;
    }

    static std::shared_ptr<Source>
    fromPath( const char* path )
    {
        const int fd = ::open( path, O_RDONLY | O_CLOEXEC );
        if ( fd < 0 ) {
            fail( MI355X_BZ2_ERR_IO, std::string( "open(" ) + path + "): " + strerror( errno ) );
        }
        return fromFd( fd, true );
    }

    static std::shared_ptr<Source>
    fromMemory( const uint8_t* bytes, uint64_t size )
    {
        auto s = std::shared_ptr<Source>( new Source() );
        s->m_copy.assign( bytes, bytes + size );
        s->m_bytes = s->m_copy.data();
        s->m_size = size;
        return s;
    }

    ~Source()
    {
        if ( m_map != nullptr ) {
            munmap( m_map, m_size );
        }
    }

    [[nodiscard]] const uint8_t* bytes() const { return m_bytes; }
    [[nodiscard]] uint64_t size() const { return m_size; }
    [[nodiscard]] uint64_t sizeInBits() const { return m_size * 8; }

private:
    Source() = default;
    const uint8_t* m_bytes{ nullptr };
    uint64_t m_size{ 0 };
    void* m_map{ nullptr };
    std::vector<uint8_t> m_copy;
};

/** MSB-first read of up to 32 bits from a byte array; sets eof if it crosses the end (BitReader.hpp:190-206). */
static uint32_t
readBits( const Source& src, uint64_t& pos, unsigned n, bool& eof )
{
    if ( pos + n > src.sizeInBits() ) {
        eof = true;
        return 0;
    }
    uint64_t v = 0;
    const uint64_t byte = pos >> 3;
    for ( int i = 0; i < 8; ++i ) {
        v = ( v << 8 ) | ( byte + i < src.size() ? src.bytes()[byte + i] : 0 );
    }
    v <<= ( pos & 7 );
    pos += n;
    return n == 0 ? 0 : (uint32_t)( v >> ( 64 - n ) );
}

/* ------------------------------------------------------------------------------------------------ host buffers */
/** Page-locked host buffers for the decoded bytes of a batch, recycled through a small pool: a pageable
 * std::vector costs a memset of the whole batch plus a staged (slow) D2H copy, pinning fresh memory per batch costs
 * more than the copy itself. */
class PinnedPool
{
public:
    struct Buffer
    {
        uint8_t* data{ nullptr };
        size_t capacity{ 0 };
    };

    ~PinnedPool()
    {
        for ( auto& b : m_free ) (void)hipHostFree( b.data );
    }

    /** A page-locked buffer of at least `size` bytes: the smallest free one that fits, else fresh memory (which costs
     * more than the copy it is for: 20 to 50 ms for a batch of 512 blocks).  `capacity`, if given, receives its size. */
    [[nodiscard]] std::shared_ptr<const uint8_t>
    get( size_t size, const std::shared_ptr<PinnedPool>& self, size_t* capacity = nullptr )
    {
        Buffer buffer;
        {
            const std::scoped_lock lock( m_mutex );
            auto best = m_free.end();
            for ( auto it = m_free.begin(); it != m_free.end(); ++it ) {
                if ( ( it->capacity >= size ) && ( best == m_free.end() || it->capacity < best->capacity ) ) best = it;
            }
            if ( best != m_free.end() ) {
                buffer = *best;
                m_free.erase( best );
            }
        }
        if ( buffer.data == nullptr ) {
            /* batches of one sequential read differ a little in size: leave headroom so that a recycled buffer fits
             * the next batch instead of pinning fresh memory */
            const size_t grain = size < ( size_t( 8 ) << 20 ) ? ( size_t( 1 ) << 20 ) : ( size_t( 16 ) << 20 );
            buffer.capacity = ( std::max<size_t>( size + size / 8, 1 ) + grain - 1 ) / grain * grain;
            if ( hipHostMalloc( reinterpret_cast<void**>( &buffer.data ), buffer.capacity, hipHostMallocDefault ) != hipSuccess ) {
                return nullptr;
            }
        }
        if ( capacity != nullptr ) *capacity = buffer.capacity;
        /* the deleter hands the memory back; the pool lives as long as any buffer does */
        return std::shared_ptr<const uint8_t>( buffer.data, [self, buffer] ( const uint8_t* ) { self->put( buffer ); } );
    }

private:
    void
    put( Buffer buffer )
    {
        const std::scoped_lock lock( m_mutex );
        if ( m_free.size() < 8 ) {
            m_free.push_back( buffer );
            return;
        }
        /* keep the larger ones */
        auto smallest = std::min_element( m_free.begin(), m_free.end(),
                                          [] ( const Buffer& a, const Buffer& b ) { return a.capacity < b.capacity; } );
        if ( smallest->capacity < buffer.capacity ) std::swap( *smallest, buffer );
        (void)hipHostFree( buffer.data );
    }

    std::mutex m_mutex;
    std::vector<Buffer> m_free;
};

/* ------------------------------------------------------------------------------------------------ decoded runs */
/** One block of a run: indexed_bzip2::BlockHeaderData / BlockData (BZ2BlockFetcher.hpp:18-34) without owning bytes. */
struct BlockRecord
{
    uint64_t bits{ 0 }, bitLength{ 0 };
    uint64_t at{ 0 }, byteLength{ 0 };       /* the block's bytes inside the run's buffer */
    uint32_t storedCrc{ 0 }, computedCrc{ 0xFFFFFFFFu };
    int status{ MI355X_BZ2_OK };
    bool endOfStream{ false }, endOfFile{ false };
};

/** Consecutive blocks [firstBlock, firstBlock + blocks.size()) of the finder's list, decoded by one batch. */
struct DecodedRun
{
    size_t firstBlock{ 0 };
    std::vector<BlockRecord> blocks;
    std::shared_ptr<const uint8_t> bytes;    /* page-locked; block k at bytes + blocks[k].at */
    size_t totalBytes{ 0 };
    bool lookAhead{ false };                 /* launched ahead of the reader (not because a read was waiting for it) */

    [[nodiscard]] size_t first() const { return firstBlock; }
    [[nodiscard]] size_t count() const { return blocks.size(); }
    [[nodiscard]] const BlockRecord& at( size_t block ) const { return blocks[block - firstBlock]; }
};

using RunPtr = std::shared_ptr<const DecodedRun>;

/** Header fields of the block at a bit offset, parsed on the host (the GPU validates the rest when it decodes it). */
struct BlockHeader
{
    uint64_t bits{ 0 }, bitLength{ 0 };
    uint32_t storedCrc{ 0 };
    bool endOfStream{ false }, endOfFile{ false };
};

/* ------------------------------------------------------------------------------------------------ batch scheduler */
class BatchScheduler
{
public:
    BatchScheduler( std::shared_ptr<Source> source, std::shared_ptr<BlockFinder> finder, size_t parallelization, int device ) :
        m_source( std::move( source ) ),
        m_finder( std::move( finder ) ),
        m_batch( std::max<size_t>( 1, parallelization ) ),
        m_contexts( contextCount( m_batch ) ),
        /* blocks that may be decoded ahead of the reader, finished or in flight: every context a full batch in flight and
         * one more queued (a context that has finished finds its next launch without waiting for the reading thread),
         * while another two are finished and being read */
        m_window( ( m_contexts + 3 ) * m_batch ),
        m_ready( m_window + std::max<size_t>( 16, m_batch ) )
    {
        /* BZ2BlockFetcher's constructor reads the stream header once: BZ2BlockFetcher.hpp:56 */
        m_level = mi355x_bz2_read_stream_header( m_source->bytes(), m_source->size(), 0 );
        if ( m_level == 0 ) {
            fail( MI355X_BZ2_ERR_STREAM_HEADER );
        }
        m_resident = fitsDevice( device );
        /* Several decoder contexts, each with its own submission thread: while one batch is copied to the host (and
         * consumed), the next ones are being decoded.  They share ONE resident copy of the compressed file.  Only the first
         * context is created here -- the first block goes to it at once; the others are created by their threads, beside
         * the first launches (a context costs tens of milliseconds: streams, events, scratch). */
        const auto tCreate = std::chrono::steady_clock::now();
        m_ctxs.assign( m_contexts, nullptr );
        {
            std::string detail;
            const int rc = createContext( device, nullptr, m_ctxs[0], detail );
            if ( rc != MI355X_BZ2_OK ) fail( rc, detail );
        }
        if ( m_trace ) {
            std::fprintf( stderr, "[reader] first context, copy of %.0f MB started: %.1f ms\n", m_source->size() / 1e6,
                          std::chrono::duration<double, std::milli>( std::chrono::steady_clock::now() - tCreate ).count() );
        }
        if ( m_resident ) {
            m_scanner = std::thread( [this] { scanOnDevice(); } );
        }
        for ( size_t i = 0; i < m_contexts; ++i ) {
            m_workers.emplace_back( [this, i, device] () {
                if ( i > 0 ) {
                    std::string detail;
                    mi355x_bz2_ctx* ctx = nullptr;
                    if ( createContext( device, m_ctxs[0], ctx, detail ) != MI355X_BZ2_OK ) {
                        const std::scoped_lock lock( m_queueMutex );
                        m_workerError = detail;
                        return;   /* the others carry on */
                    }
                    m_ctxs[i] = ctx;
                }
                workerMain( m_ctxs[i] );
            } );
        }
    }

    /** A decoder context over the file: the first one starts the copy to the GPU (in the background, in parts: the first
     * blocks decode while the rest of a large file is still on its way), the others share it. */
    int
    createContext( int device, mi355x_bz2_ctx* shareFrom, mi355x_bz2_ctx*& out, std::string& detail ) const
    {
        mi355x_bz2_config config{};
        config.device = device;
        /* scratch (10.1 MB per block) grows with the batches that are really launched: a reader that seeks and reads a
         * little never pays for a full batch, a sequential one pays once per context, on that context's own thread */
        config.max_batch_blocks = 1;
        mi355x_bz2_ctx* ctx = nullptr;
        int rc = mi355x_bz2_create( &config, &ctx );
        if ( rc != MI355X_BZ2_OK ) return rc;
        if ( m_resident ) {
            rc = shareFrom == nullptr ? mi355x_bz2_set_input_host_streamed( ctx, m_source->bytes(), m_source->size() )
                                      : mi355x_bz2_share_input( ctx, shareFrom );
        }   /* else: every launch brings the bytes of its own blocks, see workerMain */
        if ( rc != MI355X_BZ2_OK ) {
            detail = mi355x_bz2_last_error( ctx );
            mi355x_bz2_destroy( ctx );
            return rc;
        }
        out = ctx;
        return MI355X_BZ2_OK;
    }

    /**
     * Whether the whole compressed file may be kept resident on the GPU next to the decoders' scratch (the fast way: one
     * copy, the magic scan on the device).  If not -- a file beyond the free device memory, or beyond
     * MI355X_BZ2_INPUT_BUDGET bytes -- residency is BOUNDED: every launch copies the byte range of its own blocks into its
     * context's input buffer (two per context: the next range travels beside the batch in flight), the way the reference
     * streams a file through 128 KiB refills of its bit reader (src/core/BitReader.hpp:57, filereader/Shared.hpp:238-335);
     * block offsets then come from the host finder threads alone.
     */
    [[nodiscard]] bool
    fitsDevice( int device ) const
    {
        if ( const char* const budget = std::getenv( "MI355X_BZ2_INPUT_BUDGET" ) ) {
            return m_source->size() <= std::strtoull( budget, nullptr, 10 );
        }
        size_t freeBytes = 0, totalBytes = 0;
        if ( ( device >= 0 && hipSetDevice( device ) != hipSuccess ) || hipMemGetInfo( &freeBytes, &totalBytes ) != hipSuccess ) {
            return true;    /* no device: creating the first context reports that */
        }
        /* scratch and output of every context's batches, and some room for whoever else uses the device */
        const uint64_t others = (uint64_t)m_contexts * m_batch * ( uint64_t( 15 ) << 20 ) + ( uint64_t( 2 ) << 30 );
        return m_source->size() + others <= (uint64_t)freeBytes;
    }

    [[nodiscard]] bool inputResident() const { return m_resident; }

    ~BatchScheduler()
    {
        {
            const std::scoped_lock lock( m_queueMutex );
            m_stop = true;
            m_queueChanged.notify_all();
        }
        if ( m_scanner.joinable() ) m_scanner.join();
        for ( auto& worker : m_workers ) {
            if ( worker.joinable() ) worker.join();
        }
        m_flights.clear();
        for ( auto it = m_ctxs.rbegin(); it != m_ctxs.rend(); ++it ) {
            if ( *it != nullptr ) mi355x_bz2_destroy( *it );   /* owner of the input last */
        }
    }

    /** Decoder contexts for a batch size: a batch has a latency floor (its largest block), so smaller batches want more
     * of them in flight: three contexts up to 640 blocks per batch, two above; small batches keep two so that a block
     * someone waits for does not queue behind a look-ahead launch; one block at a time is the serial reader. */
    [[nodiscard]] static size_t
    contextCount( size_t batch )
    {
        if ( const char* const forced = std::getenv( "MI355X_BZ2_READER_CONTEXTS" ) ) {
            return std::min<size_t>( 4, std::max<size_t>( 1, std::strtoul( forced, nullptr, 10 ) ) );
        }
        return batch >= 64 ? ( batch <= 640 ? 3 : 2 ) : ( batch >= 2 ? 2 : 1 );
    }

    /** The fields in front of a block's tables (bzip2.hpp:479-519), read on the caller's thread: what the reader needs to
     * recognise an end-of-stream block behind a data block.  Throws like the reference's block constructor would. */
    [[nodiscard]] BlockHeader
    peekHeader( uint64_t bits ) const
    {
        BlockHeader header;
        header.bits = bits;
        uint64_t pos = bits;
        bool eof = bits > m_source->sizeInBits();
        const uint64_t magic = ( (uint64_t)readBits( *m_source, pos, 24, eof ) << 24 ) | readBits( *m_source, pos, 24, eof );
        header.storedCrc = readBits( *m_source, pos, 32, eof );
        if ( eof ) fail( MI355X_BZ2_ERR_EOF );
        if ( magic == MI355X_BZ2_MAGIC_EOS ) {
            header.endOfStream = true;
            if ( ( pos & 7 ) != 0 ) {
                readBits( *m_source, pos, 8 - (unsigned)( pos & 7 ), eof );   /* padding to the next byte */
                if ( eof ) fail( MI355X_BZ2_ERR_EOF );
            }
            header.bitLength = pos - bits;
            header.endOfFile = pos >= m_source->sizeInBits();
            return header;
        }
        if ( magic != MI355X_BZ2_MAGIC_BLOCK ) {
            char text[96];
            std::snprintf( text, sizeof( text ), "0x%llx at bit offset %llu", (unsigned long long)magic, (unsigned long long)bits );
            fail( MI355X_BZ2_ERR_BAD_MAGIC, text );
        }
        const bool randomised = readBits( *m_source, pos, 1, eof ) != 0;
        if ( eof ) fail( MI355X_BZ2_ERR_EOF );
        if ( randomised ) fail( MI355X_BZ2_ERR_RANDOMIZED );
        const uint32_t origPtr = readBits( *m_source, pos, 24, eof );
        if ( eof ) fail( MI355X_BZ2_ERR_EOF );
        if ( origPtr > 900000 ) fail( MI355X_BZ2_ERR_ORIGPTR_RANGE );
        return header;
    }

    /**
     * The run that holds block number `block` of the finder's list -- from the finished runs, from a launch in flight, or
     * from a launch of its own that goes ahead of everything queued.  Along the way: the access is noted, finished
     * launches are collected, and the range of blocks that the access pattern makes worth decoding ahead is launched.
     * A block's own failure is NOT an error here: it is in its record, for the read that needs the block.
     */
    [[nodiscard]] RunPtr
    demand( size_t block )
    {
        ++m_stats.gets;
        collectFinished();
        m_pattern.note( block );
        if ( m_pattern.inOrder() ) {
            m_ready.dropBefore( block );      /* a sequential reader never comes back (BlockFetcher.hpp:343-346) */
        }

        std::shared_future<RunPtr> pending;
        bool onDemand = false;
        RunPtr run = m_ready.find( block );
        if ( run ) {
            ++( run->lookAhead ? m_stats.prefetch_hits : m_stats.cache_hits );
        } else if ( const auto flight = flightOf( block ); flight != m_flights.end() ) {
            pending = flight->second.result;
            ++m_stats.prefetch_hits;
        } else {
            /* A batch returns when its slowest block is through: the block somebody waits for goes alone, ahead of
             * everything queued, and what should follow it as a second launch on another context. */
            ++m_stats.on_demand_fetches;
            pending = launch( block, 1, /* urgent */ true, /* lookAhead */ false );
            onDemand = true;
        }
        /* (a reader that waits for a launch in flight gains nothing from a partial launch behind it) */
        launchAhead( block, /* somebodyWaits */ onDemand );

        if ( !run ) {
            const auto tWait = std::chrono::steady_clock::now();
            run = pending.get();
            m_stats.wait_seconds += std::chrono::duration<double>( std::chrono::steady_clock::now() - tWait ).count();
            if ( !run ) {
                const std::scoped_lock lock( m_queueMutex );
                fail( MI355X_BZ2_ERR_DEVICE, m_workerError );
            }
            collectFinished();
        }
        return run;
    }

    /** Blocks that need not be consecutive, decoded once by one launch and left in the context's output for the job's
     * afterDecode, which runs on the worker's thread behind the decode and the per-block check and reports a failure by
     * throwing.  What it does there is the submitter's business (see "decode jobs" below).  A job goes ahead of
     * everything queued (somebody waits for it), publishes no run and is not a flight: the runs, flights and look-ahead
     * of the sequential reader are not disturbed. */
    struct Job
    {
        using AfterDecode = std::function<void( mi355x_bz2_ctx*, const bz2gpu::RangeLaunch& )>;

        const bz2gpu::RangeLaunch* launch{ nullptr };
        const std::atomic<bool>* cancel{ nullptr };   /* set when the job is taken: it is neither decoded nor counted */
        AfterDecode afterDecode;
        std::promise<bool> done;     /* false: cancelled; an exception if a block, the device or afterDecode failed */
    };

    [[nodiscard]] std::future<bool>
    submit( std::unique_ptr<Job> job )
    {
        auto result = job->done.get_future();
        const std::scoped_lock lock( m_queueMutex );
        m_queue.emplace_front( std::move( job ) );
        m_queueChanged.notify_all();
        return result;
    }

    [[nodiscard]] mi355x_bz2_reader_stats
    statistics() const
    {
        auto result = m_stats;
        const std::scoped_lock lock( m_queueMutex );
        result.batches = m_batches;
        result.blocks_decoded = m_blocksDecoded;
        result.decode_seconds = m_decodeSeconds;
        result.input_resident = m_resident ? 1 : 0;
        result.input_bytes_uploaded = m_uploadedBytes.load( std::memory_order_relaxed );
        return result;
    }

private:
    struct Launch
    {
        size_t first{ 0 };
        std::vector<uint64_t> offsets;
        bool lookAhead{ false };
        std::promise<RunPtr> promise;
        std::shared_ptr<std::atomic<bool> > done;
    };

    using Queued = std::variant<std::unique_ptr<Launch>, std::unique_ptr<Job> >;

    struct Flight
    {
        size_t count{ 0 };
        std::shared_future<RunPtr> result;
        std::shared_ptr<std::atomic<bool> > done;
    };

    using Flights = std::map<size_t, Flight>;   /* by first block */

    [[nodiscard]] Flights::iterator
    flightOf( size_t block )
    {
        auto behind = m_flights.upper_bound( block );
        if ( behind == m_flights.begin() ) return m_flights.end();
        --behind;
        return block - behind->first < behind->second.count ? behind : m_flights.end();
    }

    /** A thread of its own: once the whole file is resident on the GPU, let it find the block magics too (k_find_magic,
     * a few ms per GB, on a stream of its own); the host finder threads (about 1.3 GB/s of compressed data on eight
     * cores), which serve the first blocks while the copy runs, would pace the whole reader.  Same offsets, delivered at
     * once; if the scan cannot be used (more matches than its result buffer holds) the host threads carry on. */
    void
    scanOnDevice()
    {
        const auto stopped = [this] {
            const std::scoped_lock lock( m_queueMutex );
            return m_stop;
        };
        while ( mi355x_bz2_input_resident( m_ctxs.front() ) == 0 ) {
            if ( stopped() || m_finder->complete() ) return;
            std::this_thread::sleep_for( std::chrono::milliseconds( 2 ) );
        }
        if ( stopped() || m_finder->complete() ) return;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint64_t> offsets( (size_t)std::min<uint64_t>( m_source->size() / 6 + 16, 1u << 20 ) );
        uint64_t found = 0;
        if ( ( mi355x_bz2_find_magic_device( m_ctxs.front(), MI355X_BZ2_MAGIC_BLOCK, offsets.data(), offsets.size(),
                                             &found ) == MI355X_BZ2_OK ) && ( found <= offsets.size() ) ) {
            offsets.resize( found );
            /* an index given by the caller meanwhile, or a list cut behind trailing garbage, stays: decided inside the finder */
            (void)m_finder->adopt( std::vector<size_t>( offsets.begin(), offsets.end() ), BlockFinder::Authority::SCANNER );
        }
        if ( m_trace ) {
            const auto now = std::chrono::steady_clock::now();
            std::fprintf( stderr, "[reader] t=%.1f ms: file resident, magic scan %.1f ms (%zu blocks)\n",
                          std::chrono::duration<double, std::milli>( now - m_created ).count(),
                          std::chrono::duration<double, std::milli>( now - t0 ).count(), m_finder->size() );
        }
    }

    /** Launches whose worker is through move to the finished runs (one flag per launch is polled, not one future per
     * block: thousands of blocks can be in flight). */
    void
    collectFinished()
    {
        for ( auto flight = m_flights.begin(); flight != m_flights.end(); ) {
            if ( !flight->second.done->load( std::memory_order_acquire ) ) {
                ++flight;
                continue;
            }
            if ( const auto run = flight->second.result.get() ) {
                if ( run->lookAhead ) {
                    for ( const auto& record : run->blocks ) {
                        m_stats.failed_prefetches += record.status != MI355X_BZ2_OK ? 1 : 0;
                    }
                }
                m_ready.insert( run );
                m_inFlightBlocks -= flight->second.count;
                flight = m_flights.erase( flight );
            } else {
                ++flight;   /* device failure: stays, and fails whoever asks for it */
            }
        }
    }

    /** Decide from the access pattern which blocks behind `block` to decode ahead, and launch them as ONE contiguous
     * range if that is worth a launch. */
    void
    launchAhead( size_t block, bool somebodyWaits )
    {
        /* one full batch per context in flight, and one queued: launches are made on the reading thread, which may be
         * blocked on a run when a context becomes free */
        const size_t limit = m_batch * ( m_contexts + ( m_batch >= 64 ? 1 : 0 ) );
        if ( m_inFlightBlocks >= limit ) return;
        /* While a launch is kept back for want of blocks (rule at the end) a sequential reader gains about one candidate
         * per call: looking again on every call would cost O(batch^2) per batch. */
        if ( !somebodyWaits && ( m_holdOff > 0 ) && !m_flights.empty() ) {
            --m_holdOff;
            return;
        }
        const auto wanted = m_pattern.ahead( m_window );
        if ( wanted.count == 0 ) return;
        size_t end = wanted.first + wanted.count;
        if ( m_finder->complete() ) end = std::min( end, m_finder->size() );
        /* the first block of the range that is neither finished nor in flight */
        size_t from = wanted.first;
        for ( ;; ) {
            from = m_ready.firstGap( from );
            const auto flight = flightOf( from );
            if ( flight == m_flights.end() ) break;
            from = flight->first + flight->second.count;
        }
        if ( from >= end ) {
            m_holdOff = std::max<size_t>( 1, m_batch / 8 );
            return;
        }
        /* as many as fit: a batch, the room in flight, the window of blocks decoded ahead (finished ones that are still
         * wanted must not be pushed out by newer ones, BlockFetcher.hpp:527-535) */
        /* the first launches are small and grow (64, 256, 1 024 blocks): a context's scratch for a full batch (10.1 MB per block)
         * takes longer to allocate than the batch to decode, and the reader should not wait for that before its first bytes */
        size_t room = std::min( { m_batch, limit - m_inFlightBlocks, end - from, m_ramp } );
        const size_t ahead = m_ready.blocksWithin( wanted.first, end ) + m_inFlightBlocks;
        room = ahead >= m_window ? 0 : std::min( room, m_window - ahead );
        std::vector<uint64_t> offsets;
        for ( size_t b = from; b < from + room; ++b ) {
            if ( m_ready.covers( b ) || ( flightOf( b ) != m_flights.end() ) ) break;
            const auto offset = m_finder->at( b, BlockFinder::DO_NOT_WAIT ).bits;
            if ( !offset ) break;
            offsets.push_back( *offset );
        }
        if ( offsets.empty() ) {
            m_holdOff = std::max<size_t>( 1, m_batch / 8 );
            return;
        }
        /* A launch has a latency floor (its slowest block, 30 to 45 ms) whatever its size: go along with a launch somebody
         * waits for, otherwise wait until a whole batch can go (the ramp's size while the reader starts up) -- unless nothing is
         * in flight at all or the file ends here. */
        const size_t worthIt = m_batch;
        const bool reachesEnd = m_finder->complete() && ( from + offsets.size() >= m_finder->size() );
        if ( somebodyWaits || ( offsets.size() >= std::min( worthIt, m_ramp ) ) || m_flights.empty() || reachesEnd ) {
            m_ramp = std::min( m_batch, 4 * m_ramp );
            m_stats.prefetches_submitted += offsets.size();
            launch( from, std::move( offsets ), /* urgent */ false, /* lookAhead */ true );
            m_holdOff = 0;
        } else {
            m_holdOff = std::min( worthIt - offsets.size(), std::max<size_t>( 1, m_batch / 8 ) );
        }
    }

    std::shared_future<RunPtr>
    launch( size_t first, size_t count, bool urgent, bool lookAhead )
    {
        std::vector<uint64_t> offsets;
        for ( size_t b = first; b < first + count; ++b ) {
            const auto offset = m_finder->at( b ).bits;
            if ( !offset ) {
                fail( MI355X_BZ2_ERR_LOGIC, "block " + std::to_string( b ) + " is not in the block finder's list" );
            }
            offsets.push_back( *offset );
        }
        return launch( first, std::move( offsets ), urgent, lookAhead );
    }

    std::shared_future<RunPtr>
    launch( size_t first, std::vector<uint64_t> offsets, bool urgent, bool lookAhead )
    {
        auto work = std::make_unique<Launch>();
        work->first = first;
        work->offsets = std::move( offsets );
        work->lookAhead = lookAhead;
        work->done = std::make_shared<std::atomic<bool> >( false );
        Flight flight;
        flight.count = work->offsets.size();
        flight.result = work->promise.get_future().share();
        flight.done = work->done;
        m_inFlightBlocks += flight.count;
        const auto result = flight.result;
        m_flights.emplace( first, std::move( flight ) );
        {
            const std::scoped_lock lock( m_queueMutex );
            if ( urgent ) {
                m_queue.push_front( std::move( work ) );   /* someone is waiting for it */
            } else {
                m_queue.push_back( std::move( work ) );
            }
            m_queueChanged.notify_all();
        }
        return result;
    }

    /** One submission thread per decoder context: takes a launch, decodes the batch, copies it to a page-locked buffer,
     * publishes the run.  Replaces the thread pool of per-block tasks (BlockFetcher.hpp:620-642).
     * The copy of a batch runs in the background while the context's next batch is launched (the context writes to a
     * second output buffer meanwhile), and the page-locked buffer is fetched while the GPU is decoding. */
    void
    workerMain( mi355x_bz2_ctx* const ctx )
    {
        struct Step
        {
            std::unique_ptr<Launch> work;
            std::vector<mi355x_bz2_block_result> results;
            std::shared_ptr<const uint8_t> buffer;
            uint64_t total{ 0 };
            std::chrono::steady_clock::time_point t0;
        };
        const auto failStep = [this, ctx] ( Step& step ) {
            {
                const std::scoped_lock lock( m_queueMutex );
                m_workerError = mi355x_bz2_last_error( ctx );
            }
            step.work->promise.set_value( nullptr );
            step.work->done->store( true, std::memory_order_release );
        };
        /* the copy of `step` has been queued: wait for it and hand the run over */
        const auto publish = [this, ctx, &failStep] ( Step& step ) {
            if ( mi355x_bz2_copy_output_end( ctx ) != MI355X_BZ2_OK ) {
                failStep( step );
                return;
            }
            const auto n = step.results.size();
            auto run = std::make_shared<DecodedRun>();
            run->firstBlock = step.work->first;
            run->bytes = std::move( step.buffer );
            run->totalBytes = step.total;
            run->lookAhead = step.work->lookAhead;
            run->blocks.resize( n );
            for ( size_t i = 0; i < n; ++i ) {
                const auto& r = step.results[i];
                auto& record = run->blocks[i];
                record.bits = step.work->offsets[i];
                record.bitLength = r.encoded_size_bits;
                record.storedCrc = r.header_crc;
                record.computedCrc = r.computed_crc;
                record.endOfStream = r.is_eos != 0;
                record.endOfFile = r.is_eof != 0;
                record.status = r.status;
                if ( r.status == MI355X_BZ2_OK ) {
                    record.at = r.data_offset;
                    record.byteLength = r.decoded_size;
                }
            }
            step.work->promise.set_value( std::move( run ) );
            step.work->done->store( true, std::memory_order_release );
            const std::scoped_lock lock( m_queueMutex );
            ++m_batches;
            m_blocksDecoded += n;
            m_decodeSeconds += std::chrono::duration<double>( std::chrono::steady_clock::now() - step.t0 ).count();
        };

        std::optional<Step> copying;    /* decoded, on its way to the host */

        /* A job.  Ordering against the run of this context that may still be on its way to the host (`copying`): that
         * copy reads the output buffer of the context's previous batch, on the context's copy stream.
         * decode_batch_begin sees the copy and puts this batch into the context's other output buffer; while this batch
         * decodes, the copy is waited for and its run published; decode_batch_end then leaves this batch's buffer as the
         * context's output, which afterDecode reads with calls that return only when their results are where they
         * belong.  Nothing reads this buffer afterwards, so the context's next batch may write into it at once. */
        const auto runJob = [&] ( Job& job ) {
            if ( job.cancel != nullptr && job.cancel->load( std::memory_order_acquire ) ) {
                job.done.set_value( false );
                return;
            }
            const auto t0 = std::chrono::steady_clock::now();
            const auto& launch = *job.launch;
            const auto n = (uint32_t)launch.bits.size();
            std::vector<mi355x_bz2_block_result> results( n );
            std::shared_ptr<const uint8_t> staging;   /* bounded residency: the packed windows, page-locked */
            int rc = MI355X_BZ2_OK;
            if ( m_resident ) {
                rc = mi355x_bz2_decode_batch_begin( ctx, launch.bits.data(), n );
            } else {
                staging = m_hostBuffers->get( (size_t)launch.packedBytes, m_hostBuffers );
                if ( !staging ) {
                    rc = MI355X_BZ2_ERR_DEVICE;
                } else {
                    auto* const bytes = const_cast<uint8_t*>( staging.get() );
                    uint64_t end = 0;
                    for ( const auto& window : launch.windows ) {
                        std::memset( bytes + end, 0, window.at - end );
                        std::memcpy( bytes + window.at, m_source->bytes() + window.from, window.to - window.from );
                        end = window.at + ( window.to - window.from );
                    }
                    rc = mi355x_bz2_set_input_host_async( ctx, bytes, launch.packedBytes );
                    if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_decode_batch_begin( ctx, launch.packedBits.data(), n );
                    m_uploadedBytes.fetch_add( launch.packedBytes, std::memory_order_relaxed );
                }
            }
            if ( copying ) {
                publish( *copying );
                copying.reset();
            }
            uint64_t total = 0;
            if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_decode_batch_end( ctx, results.data(), &total );
            std::exception_ptr failure;
            try {
                checkDevice( ctx, rc );
                for ( uint32_t k = 0; k < n; ++k ) {
                    const auto& r = results[k];
                    if ( r.status != MI355X_BZ2_OK ) {
                        fail( r.status, "block at bit offset " + std::to_string( launch.bits[k] ) );
                    } else if ( r.decoded_size != launch.sizes[k] || r.data_offset != launch.outOffsets[k] ) {
                        fail( MI355X_BZ2_ERR_LOGIC, "the block index promises more bytes than the block decodes to" );
                    }
                }
                job.afterDecode( ctx, launch );
            } catch ( ... ) {
                failure = std::current_exception();
            }
            staging.reset();
            {
                const std::scoped_lock lock( m_queueMutex );
                ++m_batches;
                m_blocksDecoded += n;
                m_decodeSeconds += std::chrono::duration<double>( std::chrono::steady_clock::now() - t0 ).count();
            }
            if ( failure ) {
                job.done.set_exception( failure );
            } else {
                job.done.set_value( true );
            }
        };

        while ( true ) {
            Queued next;
            {
                std::unique_lock lock( m_queueMutex );
                if ( copying && m_queue.empty() && !m_stop ) {
                    /* nothing to launch beside the copy: finish it first, somebody may be waiting for exactly this run */
                    lock.unlock();
                    publish( *copying );
                    copying.reset();
                    lock.lock();
                }
                m_queueChanged.wait( lock, [this] { return m_stop || !m_queue.empty(); } );
                if ( m_queue.empty() ) {
                    break;   /* m_stop */
                }
                next = std::move( m_queue.front() );
                m_queue.pop_front();
            }
            if ( const auto* const job = std::get_if<std::unique_ptr<Job> >( &next ) ) {
                runJob( **job );
                continue;
            }
            Step step;
            step.work = std::move( std::get<std::unique_ptr<Launch> >( next ) );
            step.t0 = std::chrono::steady_clock::now();
            const auto n = (uint32_t)step.work->offsets.size();
            step.results.resize( n );
            int rc = MI355X_BZ2_OK;
            if ( m_resident ) {
                rc = mi355x_bz2_decode_batch_begin( ctx, step.work->offsets.data(), n );
            } else {
                /* bounded residency: the bytes from the word of the first block's magic to where the last block can end at
                 * the latest (900 000 symbols of 20 bits and the tables in front of them: below 2 400 000 bytes), and the
                 * blocks' offsets inside that range.  The copy is queued on the context's input stream; while a batch of
                 * this context is still being copied out, it lands in the context's second input buffer. */
                const auto [lowest, highest] = std::minmax_element( step.work->offsets.begin(), step.work->offsets.end() );
                const uint64_t from = ( *lowest / 8 ) & ~uint64_t( 3 );
                const uint64_t to = std::min<uint64_t>( m_source->size(), *highest / 8 + 2400000 );
                std::vector<uint64_t> relative( step.work->offsets );
                for ( auto& bits : relative ) bits -= 8 * from;
                rc = from < to ? mi355x_bz2_set_input_host_async( ctx, m_source->bytes() + from, to - from )
                               : MI355X_BZ2_ERR_INVALID_ARGUMENT;
                if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_decode_batch_begin( ctx, relative.data(), n );
                m_uploadedBytes.fetch_add( to - from, std::memory_order_relaxed );
            }
            const auto t1 = std::chrono::steady_clock::now();
            /* while the GPU works: the run in front of this one, and the memory for this one (a block of the usual
             * compressors decodes to at most level x 100 000 bytes; if these decode to more -- later streams of the file
             * may have a higher level -- a second buffer is fetched below) */
            if ( copying ) {
                publish( *copying );
                copying.reset();
            }
            size_t capacity = 0;
            if ( rc == MI355X_BZ2_OK ) {
                step.buffer = m_hostBuffers->get( (size_t)n * m_level * 100000 + 4096, m_hostBuffers, &capacity );
            }
            const auto t2 = std::chrono::steady_clock::now();
            if ( rc == MI355X_BZ2_OK ) {
                rc = mi355x_bz2_decode_batch_end( ctx, step.results.data(), &step.total );
            }
            const auto t3 = std::chrono::steady_clock::now();
            if ( rc == MI355X_BZ2_OK ) {
                if ( step.total > capacity ) step.buffer = m_hostBuffers->get( step.total, m_hostBuffers );
                if ( !step.buffer ) {
                    rc = MI355X_BZ2_ERR_DEVICE;
                } else {
                    rc = mi355x_bz2_copy_output_begin( ctx, 0, step.total, const_cast<uint8_t*>( step.buffer.get() ) );
                }
            }
            if ( m_trace ) {
                const auto ms = [] ( auto a, auto b ) { return std::chrono::duration<double, std::milli>( b - a ).count(); };
                std::fprintf( stderr, "[reader] t=%.1f ms: blocks [%zu, +%u) on ctx %p: launch %.1f ms, previous run + host "
                              "buffer %.1f ms, rest of the decode %.1f ms, %.0f MB\n", ms( m_created, step.t0 ),
                              step.work->first, n, (void*)ctx, ms( step.t0, t1 ), ms( t1, t2 ), ms( t2, t3 ), step.total / 1e6 );
            }
            if ( rc != MI355X_BZ2_OK ) {
                failStep( step );
                continue;
            }
            copying = std::move( step );
        }
        if ( copying ) publish( *copying );
    }

private:
    const std::shared_ptr<Source> m_source;
    const std::shared_ptr<BlockFinder> m_finder;
    const size_t m_batch;        /* blocks per launch = the `parallelization` of the API */
    const size_t m_contexts;
    const size_t m_window;

    SequentialityTracker m_pattern;
    RunCache<DecodedRun> m_ready;
    Flights m_flights;
    size_t m_inFlightBlocks{ 0 };
    size_t m_holdOff{ 0 };
    size_t m_ramp{ 64 };         /* blocks of the next look-ahead launch while the reader is starting up */
    unsigned m_level{ 9 };       /* of the first stream: 100 000 bytes per block and level */
    bool m_resident{ true };     /* the whole compressed file on the GPU, or the range of every launch (fitsDevice) */
    std::atomic<uint64_t> m_uploadedBytes{ 0 };

    std::vector<mi355x_bz2_ctx*> m_ctxs;
    const std::shared_ptr<PinnedPool> m_hostBuffers{ std::make_shared<PinnedPool>() };
    std::vector<std::thread> m_workers;
    std::thread m_scanner;       /* see scanOnDevice */
    mutable std::mutex m_queueMutex;
    std::condition_variable m_queueChanged;
    std::deque<Queued> m_queue;
    bool m_stop{ false };
    const bool m_trace{ std::getenv( "MI355X_BZ2_READER_TRACE" ) != nullptr };
    const std::chrono::steady_clock::time_point m_created{ std::chrono::steady_clock::now() };
    std::string m_workerError;
    uint64_t m_batches{ 0 };
    uint64_t m_blocksDecoded{ 0 };
    double m_decodeSeconds{ 0 };

    mi355x_bz2_reader_stats m_stats{};
};

/* ------------------------------------------------------------------------------------------------ decode jobs */
/* What the reader's positionless calls do with a launch's blocks once they lie decoded in the context's output: the
 * afterDecode of BatchScheduler::Job.  Each of these runs on the worker thread of the context it is given, reports a
 * failure by throwing, and reads and writes memory of the call that submitted it (StreamReader::runJobs waits). */

/** read_ranges: the launch's pieces, straight into the caller's destination. */
static void
gatherPieces( mi355x_bz2_ctx* const ctx, const std::vector<mi355x_bz2_gather_piece>& pieces, void* dst, bool dstIsDevice )
{
    checkDevice( ctx, mi355x_bz2_gather_output( ctx, pieces.data(), (uint32_t)pieces.size(), dst, dstIsDevice ? 1 : 0 ) );
}

/** A piece of a line range, packed into the result buffer of the context that decoded it (step 1 of
 * read_line_ranges), where it stays until step 2 puts it in place. */
struct HeldPiece
{
    mi355x_bz2_ctx* ctx{ nullptr };
    uint32_t range{ 0 };
    uint64_t offset{ 0 }, size{ 0 };
};

/** How many bytes of each context's result buffer are held for read_line_ranges.  The launches of a call run on
 * several contexts at once, each on its context's thread: every access under the mutex. */
struct HeldBytes
{
    std::mutex mutex;
    std::map<mi355x_bz2_ctx*, uint64_t> of;
};

[[noreturn]] static void
failLyingLineIndex( uint64_t blockStart, uint64_t promised, uint64_t counted )
{
    fail( MI355X_BZ2_ERR_LOGIC, "the line index gives the block at decoded offset " + std::to_string( blockStart ) + " "
                                + std::to_string( promised ) + " delimiters, it holds " + std::to_string( counted ) );
}

/** What a launch of the line functions does with its decoded blocks, in this order: count `nl` in every block (the
 * line index), find the plan's boundary queries of this launch (positions[query], an array all launches of the call
 * share), resolve the launch's segments with them and pack the pieces behind what the context already holds. */
struct LineWork
{
    uint8_t nl{ 0 };
    bool countBlocks{ false };
    std::vector<uint64_t> blockCounts;          /* out: per block of the launch */
    const bz2gpu::LinePlan* plan{ nullptr };
    std::vector<uint32_t> queries, segments;    /* of this launch: indexes into the plan's lists */
    uint64_t* positions{ nullptr };
    std::vector<HeldPiece> held;                /* out: one per segment that has bytes */
};

static void
runLineWork( mi355x_bz2_ctx* const ctx, const bz2gpu::RangeLaunch& launch, LineWork& work, HeldBytes& heldBytes )
{
    if ( work.countBlocks ) {
        std::vector<mi355x_bz2_byte_span> spans( launch.bits.size() );
        for ( size_t k = 0; k < spans.size(); ++k ) spans[k] = { launch.outOffsets[k], launch.sizes[k] };
        work.blockCounts.assign( spans.size(), 0 );
        checkDevice( ctx, mi355x_bz2_count_byte( ctx, spans.data(), (uint32_t)spans.size(), work.nl, work.blockCounts.data() ) );
    }
    if ( !work.queries.empty() ) {
        std::vector<mi355x_bz2_byte_query> queries( work.queries.size() );
        std::vector<uint64_t> found( queries.size() );
        for ( size_t k = 0; k < queries.size(); ++k ) {
            const auto& q = work.plan->queries[work.queries[k]];
            queries[k] = { q.spanOffset, q.spanSize, q.rank };
        }
        /* an index that gives a queried block another count than the block has would cut lines in the wrong places */
        std::vector<mi355x_bz2_byte_span> spans( queries.size() );
        std::vector<uint64_t> counted( queries.size() );
        for ( size_t k = 0; k < queries.size(); ++k ) spans[k] = { queries[k].offset, queries[k].size };
        checkDevice( ctx, mi355x_bz2_count_byte( ctx, spans.data(), (uint32_t)spans.size(), work.nl, counted.data() ) );
        checkDevice( ctx, mi355x_bz2_find_byte( ctx, queries.data(), (uint32_t)queries.size(), work.nl, found.data() ) );
        for ( size_t k = 0; k < queries.size(); ++k ) {
            const auto& q = work.plan->queries[work.queries[k]];
            work.positions[work.queries[k]] = found[k];
            if ( found[k] == bz2gpu::NOT_FOUND || counted[k] != q.blockCount ) {
                failLyingLineIndex( q.blockStart, q.blockCount, counted[k] );
            }
        }
    }
    if ( work.segments.empty() ) return;
    std::vector<mi355x_bz2_gather_piece> pieces;
    uint64_t base = 0;
    {
        const std::scoped_lock lock( heldBytes.mutex );
        base = heldBytes.of[ctx];
    }
    uint64_t at = base;
    for ( const auto index : work.segments ) {
        const auto& segment = work.plan->segments[index];
        uint64_t src = 0, size = 0;
        if ( !bz2gpu::resolveSegment( *work.plan, segment, work.positions, &src, &size ) ) {
            fail( MI355X_BZ2_ERR_LOGIC, "the line index contradicts the decoded data" );
        }
        if ( size == 0 ) continue;
        pieces.push_back( { src, at, size } );
        work.held.push_back( { ctx, segment.range, at, size } );
        at += size;
    }
    if ( at == base ) return;
    uint8_t* held = nullptr;
    checkDevice( ctx, resultBuffer( ctx, at, base, &held ) );
    checkDevice( ctx, mi355x_bz2_gather_output( ctx, pieces.data(), (uint32_t)pieces.size(), held, 1 ) );
    const std::scoped_lock lock( heldBytes.mutex );
    heldBytes.of[ctx] = at;
}

/** What a launch of line_numbers does with its decoded blocks: mi355x_bz2_rank_byte for the plan's queries of this
 * launch, queries [first, first + count) -- the planner lists them launch by launch --, into ranks[query], an array
 * all launches of the call share.  The rank at the end of a block's span is the block's count: an index that says
 * otherwise does not fit the data. */
struct RankWork
{
    uint8_t nl{ 0 };
    const bz2gpu::LineNumberPlan* plan{ nullptr };
    size_t first{ 0 }, count{ 0 };
    uint64_t* ranks{ nullptr };
};

static void
runRankWork( mi355x_bz2_ctx* const ctx, const RankWork& work )
{
    if ( work.count == 0 ) return;
    if ( work.count > std::numeric_limits<uint32_t>::max() ) {
        fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "line_numbers: too many offsets in one launch" );
    }
    std::vector<mi355x_bz2_rank_query> queries( work.count );
    for ( size_t k = 0; k < work.count; ++k ) {
        const auto& q = work.plan->queries[work.first + k];
        queries[k] = { q.spanOffset, q.spanSize, q.position };
    }
    uint64_t* const ranks = work.ranks + work.first;
    checkDevice( ctx, mi355x_bz2_rank_byte( ctx, queries.data(), (uint32_t)queries.size(), work.nl, ranks ) );
    for ( size_t k = 0; k < work.count; ++k ) {
        const auto& q = work.plan->queries[work.first + k];
        if ( q.expected != bz2gpu::NOT_FOUND && ranks[k] != q.expected ) failLyingLineIndex( q.blockStart, q.expected, ranks[k] );
    }
}

/** How far a search with a limit has come: what the launches at the front of the range that are through have found.
 * Once that reaches the limit, `stop` cancels the launches that have not been started. */
struct SearchProgress
{
    std::mutex mutex;
    std::vector<uint8_t> finished;              /* per launch */
    std::vector<uint64_t> values;               /* per launch: what it adds to `found` */
    size_t through{ 0 };                        /* launches [0, through) are finished ... */
    uint64_t found{ 0 };                        /* ... and have found this many */
    std::atomic<bool> stop{ false };

    explicit SearchProgress( size_t launches ) : finished( launches, 0 ), values( launches, 0 ) {}

    /** Launch `index` is through and adds `value`. */
    void
    finish( size_t index, uint64_t value, uint64_t limit )
    {
        const std::scoped_lock lock( mutex );
        finished[index] = 1;
        values[index] = value;
        while ( through < finished.size() && finished[through] != 0 ) found += values[through++];
        if ( found >= limit ) stop.store( true, std::memory_order_release );
    }
};

/** The seams of the first `usable` works of a search for patterns of at most m bytes: the first and the last
 * seamLength( m, size ) bytes of every extent, which its launch left in the work's `seam`. */
template<typename Work>
static std::vector<bz2gpu::ExtentSeam>
extentSeams( const std::vector<Work>& works, size_t usable, uint32_t m )
{
    std::vector<bz2gpu::ExtentSeam> seams( usable );
    for ( size_t l = 0; l < usable; ++l ) {
        const auto& extent = works[l].extent;
        const auto* const head = works[l].seam;
        const auto* const tail = head + bz2gpu::SEARCH_PATTERN_MAX;
        const auto k = bz2gpu::seamLength( m, extent.size );
        seams[l] = { extent.fileOffset, extent.size, { head, head + k }, { tail, tail + k } };
    }
    return seams;
}

/** What the launches of one search share: the pattern (folded once here if the flags ask for it; the context folds what
 * it uploads all the same), the flags, and -- with a limit -- the progress, which counts every match of a launch. */
struct SearchCall
{
    std::vector<uint8_t> pattern;
    uint32_t flags{ 0 };                        /* MI355X_BZ2_SEARCH_* */
    uint64_t limit{ 0 };                        /* 0: count only */
    SearchProgress progress;
};

/** What a launch of a search does with its decoded blocks: mi355x::searchOutput over its extent. */
struct SearchWork
{
    SearchCall* call{ nullptr };
    uint32_t index{ 0 };
    bz2gpu::SearchExtent extent;
    uint64_t count{ 0 };                        /* out: matches inside the extent */
    std::vector<uint64_t> positions;            /* out (limit > 0): the first min( count, limit ), in the launch's output */
    uint8_t seam[2 * bz2gpu::SEARCH_PATTERN_MAX]{};   /* out: head at 0, tail at SEARCH_PATTERN_MAX */
};

static void
runSearchWork( mi355x_bz2_ctx* const ctx, SearchWork& work )
{
    auto& call = *work.call;
    checkDevice( ctx, searchOutput( ctx, { work.extent.src, work.extent.size }, call.pattern.data(), (uint32_t)call.pattern.size(),
                                    call.flags, call.limit, call.limit > 0 ? &work.positions : nullptr, &work.count, work.seam ) );
    if ( call.limit > 0 ) call.progress.finish( work.index, work.count, call.limit );
}

/** SearchCall for a set of patterns; the set holds the flag and the patterns folded once.  The progress counts, of the
 * pairs of a launch, only those that end m_max bytes in front of its extent's end (bz2_search.hpp: the limit of a set). */
struct SetSearchCall
{
    const bz2gpu::PatternSet* set{ nullptr };
    uint64_t limit{ 0 };                        /* 0: count only */
    SearchProgress progress;
};

struct SetSearchWork
{
    SetSearchCall* call{ nullptr };
    uint32_t index{ 0 };
    bz2gpu::SearchExtent extent;
    uint64_t count{ 0 };                        /* out: pairs inside the extent */
    std::vector<uint64_t> perPattern;           /* out (limit == 0): per pattern */
    std::vector<uint64_t> positions;            /* out (limit > 0): the first min( count, limit ) pairs, positions in D */
    std::vector<uint32_t> ids;
    uint8_t seam[2 * bz2gpu::SEARCH_PATTERN_MAX]{};   /* out: head at 0, tail at SEARCH_PATTERN_MAX */
};

static void
runSetSearchWork( mi355x_bz2_ctx* const ctx, SetSearchWork& work )
{
    auto& call = *work.call;
    const bool pairs = call.limit > 0;
    if ( !pairs ) work.perPattern.assign( call.set->count(), 0 );
    checkDevice( ctx, searchOutputSet( ctx, { work.extent.src, work.extent.size }, *call.set, call.limit,
                                       pairs ? &work.positions : nullptr, pairs ? &work.ids : nullptr, &work.count,
                                       pairs ? nullptr : work.perPattern.data(), work.seam ) );
    if ( pairs ) {
        for ( auto& position : work.positions ) position = work.extent.fileOffset + ( position - work.extent.src );
        call.progress.finish( work.index, bz2gpu::safePairs( work.positions.data(), work.positions.size(),
                                                             work.extent.fileOffset + work.extent.size, call.set->mMax ), call.limit );
    }
}

/* The per-line column queries, as StreamReader::lineColumns takes them: COLUMNS device columns of one 8-byte word per
 * line; the stretch type of the stitcher and where a stretch's size goes; pass() does one stretch on the context that
 * decoded it, writing the lines of `place` at to[c] (the column's pointer at place.at), and returns the number of lines it
 * found the stretch to close; stitch() is the stitcher; words() is a stitched value as its line's word in every column,
 * and tail() the unterminated tail of what the stitcher returned. */
using ColumnPiece = bz2gpu::LineHashPlan::Piece;

struct LineHashQuery
{
    static constexpr size_t COLUMNS = 1;        /* hashes */
    using Stretch = bz2gpu::HashStretch;
    uint8_t nl;
    uint64_t x;

    static uint64_t& size( Stretch& stretch ) { return stretch.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, hashLinesOutput( ctx, { piece.src, piece.size }, nl, x, place.skip, place.take, to[0], &stretch.summary ) );
        return stretch.summary.count;
    }

    template<typename Patch>
    auto stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const { return bz2gpu::stitchSummaries( stretches, patch ); }

    static std::array<uint64_t, COLUMNS> words( uint64_t hash ) { return { hash }; }
    static uint64_t tail( const bz2gpu::StitchedHashes& stitched ) { return stitched.tailHash; }
};

struct FieldSpanQuery
{
    static constexpr size_t COLUMNS = 2;        /* starts, sizes (int64) */
    using Stretch = bz2gpu::FieldStretch;
    uint8_t nl, dl;
    uint32_t field;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldSpansOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, field, place.skip, place.take,
                                            to[0], reinterpret_cast<int64_t*>( to[1] ), &stretch.summary ) );
        return stretch.summary.count;
    }

    template<typename Patch>
    auto stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const { return bz2gpu::stitchFields( stretches, field, patch ); }

    static std::array<uint64_t, COLUMNS> words( const bz2gpu::FieldSpan& span ) { return { span.start, (uint64_t)span.size }; }
    static const bz2gpu::FieldSpan& tail( const bz2gpu::StitchedFields& stitched ) { return stitched.tail; }
};

/** FieldSpanQuery under a quote: the launches write contents, the stitcher's patches and tail are raw fields, which the
 * reader trims (StreamReader::quotedContents). */
struct QuotedFieldSpanQuery
{
    static constexpr size_t COLUMNS = 2;        /* starts, sizes (int64) */
    using Stretch = bz2gpu::QuotedFieldStretch;
    uint8_t nl, dl, quote;
    uint32_t field;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldSpansQuotedOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, quote, field, place.skip,
                                                  place.take, to[0], reinterpret_cast<int64_t*>( to[1] ), &stretch.summary ) );
        return stretch.summary.count;
    }

    template<typename Patch>
    auto stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const { return bz2gpu::stitchQuotedFields( stretches, field, patch ); }

    static std::array<uint64_t, COLUMNS> words( const bz2gpu::FieldSpan& span ) { return { span.start, (uint64_t)span.size }; }
    static const bz2gpu::FieldSpan& tail( const bz2gpu::StitchedFields& stitched ) { return stitched.tail; }
};

struct FieldHashQuery
{
    static constexpr size_t COLUMNS = 3;        /* keys, starts, sizes (int64) */
    using Stretch = bz2gpu::FieldHashStretch;
    uint8_t nl, dl;
    uint32_t field;
    uint64_t x;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.fields.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldHashesOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, field, x, place.skip, place.take,
                                             to[0], to[1], reinterpret_cast<int64_t*>( to[2] ), &stretch.summary ) );
        return stretch.summary.fields.count;
    }

    template<typename Patch>
    auto
    stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const
    {
        return bz2gpu::stitchFieldHashes( stretches, x, dl, field, patch );
    }

    static std::array<uint64_t, COLUMNS>
    words( const bz2gpu::FieldKey& key )
    {
        return { key.key, key.field.start, (uint64_t)key.field.size };
    }

    static const bz2gpu::FieldKey& tail( const bz2gpu::StitchedFieldHashes& stitched ) { return stitched.tail; }
};

struct FieldNumberQuery
{
    static constexpr size_t COLUMNS = 3;        /* numbers (int64), starts, sizes (int64) */
    using Stretch = bz2gpu::FieldNumberStretch;
    uint8_t nl, dl;
    uint32_t field;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.fields.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldNumbersOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, field, place.skip, place.take,
                                              reinterpret_cast<int64_t*>( to[0] ), to[1], reinterpret_cast<int64_t*>( to[2] ),
                                              &stretch.summary ) );
        return stretch.summary.fields.count;
    }

    /** stitchFieldNumbers with a line's number and field as one value, as lineColumns patches them. */
    struct Stitched
    {
        uint64_t closed{ 0 };
        bool hasTail{ false };
        bz2gpu::FieldNumber tail;
    };

    template<typename Patch>
    Stitched
    stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const
    {
        const auto stitched = bz2gpu::stitchFieldNumbers( stretches, field, [&patch] ( uint64_t k, int64_t number, const bz2gpu::FieldSpan& span ) {
            patch( k, bz2gpu::FieldNumber{ number, span } );
        } );
        return { stitched.closed, stitched.hasTail, { stitched.tailNumber, stitched.tail } };
    }

    static std::array<uint64_t, COLUMNS>
    words( const bz2gpu::FieldNumber& number )
    {
        return { (uint64_t)number.number, number.field.start, (uint64_t)number.field.size };
    }

    static const bz2gpu::FieldNumber& tail( const Stitched& stitched ) { return stitched.tail; }
};

/* field_sums: the key of one field and the number of another per line, from ONE decode: both passes run over the stretch
 * while it is resident, and both stitchers over the summaries; their patches name the same lines. */
struct FieldSumQuery
{
    static constexpr size_t COLUMNS = 4;        /* keys, the key field's starts and sizes (int64), values (int64) */
    struct Stretch
    {
        uint64_t fileOffset{ 0 }, size{ 0 };
        bz2gpu::FieldHashSummary keys;
        bz2gpu::FieldNumberSummary values;
    };
    struct Value
    {
        bz2gpu::FieldKey key;
        int64_t number{ bz2gpu::FIELD_NUMBER_MISSING };
    };
    struct Stitched
    {
        uint64_t closed{ 0 };
        bool hasTail{ false };
        Value tail;
    };
    uint8_t nl, dl;
    uint32_t keyField, valueField;
    uint64_t x;

    static uint64_t& size( Stretch& stretch ) { return stretch.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldHashesOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, keyField, x, place.skip, place.take,
                                             to[0], to[1], reinterpret_cast<int64_t*>( to[2] ), &stretch.keys ) );
        checkDevice( ctx, fieldNumbersOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, valueField, place.skip, place.take,
                                              reinterpret_cast<int64_t*>( to[3] ), nullptr, nullptr, &stretch.values ) );
        if ( stretch.keys.fields.count != stretch.values.fields.count ) {
            fail( MI355X_BZ2_ERR_LOGIC, "field_sums: the two passes over one stretch count different lines" );
        }
        return stretch.keys.fields.count;
    }

    template<typename Patch>
    Stitched
    stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const
    {
        std::vector<bz2gpu::FieldHashStretch> keys( stretches.size() );
        std::vector<bz2gpu::FieldNumberStretch> values( stretches.size() );
        for ( size_t i = 0; i < stretches.size(); ++i ) {
            keys[i] = { stretches[i].fileOffset, stretches[i].keys };
            values[i] = { stretches[i].fileOffset, stretches[i].values };
            keys[i].summary.fields.size = values[i].summary.fields.size = stretches[i].size;
        }
        std::vector<std::pair<uint64_t, bz2gpu::FieldKey> > keyPatches;
        const auto stitchedKeys = bz2gpu::stitchFieldHashes( keys, x, dl, keyField, [&] ( uint64_t k, const bz2gpu::FieldKey& key ) {
            keyPatches.emplace_back( k, key );
        } );
        size_t next = 0;
        const auto stitchedValues = bz2gpu::stitchFieldNumbers( values, valueField, [&] ( uint64_t k, int64_t number, const bz2gpu::FieldSpan& ) {
            if ( next >= keyPatches.size() || keyPatches[next].first != k ) {
                fail( MI355X_BZ2_ERR_LOGIC, "field_sums: the two stitchers patch different lines" );
            }
            patch( k, Value{ keyPatches[next++].second, number } );
        } );
        if ( next != keyPatches.size() || stitchedKeys.closed != stitchedValues.closed || stitchedKeys.hasTail != stitchedValues.hasTail ) {
            fail( MI355X_BZ2_ERR_LOGIC, "field_sums: the two stitchers disagree about the lines" );
        }
        return { stitchedKeys.closed, stitchedKeys.hasTail, { stitchedKeys.tail, stitchedValues.tailNumber } };
    }

    static std::array<uint64_t, COLUMNS>
    words( const Value& value )
    {
        return { value.key.key, value.key.field.start, (uint64_t)value.key.field.size, (uint64_t)value.number };
    }

    static const Value& tail( const Stitched& stitched ) { return stitched.tail; }
};

/* field_matches: field_hashes' three columns and a flag per line, from ONE decode: behind the field-hash pass, while the
 * stretch is resident, k_field_match compares the fields whose key and size hit the value table with the values' bytes
 * (matchFieldsOutput).  The stitcher is field_hashes': a line that crosses a seam and the tail get the flag 0 here, and
 * StreamReader::fieldMatches decides them from their bytes. */
struct FieldMatchQuery
{
    static constexpr size_t COLUMNS = 4;        /* keys, starts, sizes (int64), flags */
    using Stretch = bz2gpu::FieldHashStretch;
    uint8_t nl, dl;
    uint32_t field;
    uint64_t x;
    const bz2gpu::ValueTable* table;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.fields.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldHashesOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, field, x, place.skip, place.take,
                                             to[0], to[1], reinterpret_cast<int64_t*>( to[2] ), &stretch.summary ) );
        const uint64_t closed = stretch.summary.fields.count;
        const uint64_t written = closed > place.skip ? std::min( closed - place.skip, place.take ) : 0;
        checkDevice( ctx, matchFieldsOutput( ctx, *table, to[0], to[1], reinterpret_cast<const int64_t*>( to[2] ), written, piece.src,
                                             piece.fileOffset, to[3] ) );
        return closed;
    }

    template<typename Patch>
    auto
    stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const
    {
        return bz2gpu::stitchFieldHashes( stretches, x, dl, field, patch );
    }

    static std::array<uint64_t, COLUMNS>
    words( const bz2gpu::FieldKey& key )
    {
        return { key.key, key.field.start, (uint64_t)key.field.size, 0 };
    }

    static const bz2gpu::FieldKey& tail( const bz2gpu::StitchedFieldHashes& stitched ) { return stitched.tail; }
};

/* field_matches_regex: field_spans' two columns and a flag per line, from ONE decode: behind the field-span pass, while the
 * stretch is resident, k_field_regex runs the automaton over the fields of the lines written (matchFieldsRegexOutput).  The
 * stretch and the stitcher are field_spans': a line that crosses a seam and the tail get the flag 0 here, and
 * StreamReader::fieldMatchesRegex decides them from their bytes. */
struct FieldRegexQuery
{
    static constexpr size_t COLUMNS = 3;        /* starts, sizes (int64), flags */
    using Stretch = bz2gpu::FieldStretch;
    uint8_t nl, dl;
    uint32_t field;
    const bz2gpu::Regex* regex;

    static uint64_t& size( Stretch& stretch ) { return stretch.summary.size; }

    uint64_t
    pass( mi355x_bz2_ctx* ctx, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place, const std::array<uint64_t*, COLUMNS>& to,
          Stretch& stretch ) const
    {
        checkDevice( ctx, fieldSpansOutput( ctx, { piece.src, piece.size }, piece.fileOffset, nl, dl, field, place.skip, place.take,
                                            to[0], reinterpret_cast<int64_t*>( to[1] ), &stretch.summary ) );
        const uint64_t closed = stretch.summary.count;
        const uint64_t written = closed > place.skip ? std::min( closed - place.skip, place.take ) : 0;
        checkDevice( ctx, matchFieldsRegexOutput( ctx, *regex, to[0], reinterpret_cast<const int64_t*>( to[1] ), written, piece.src,
                                                  piece.fileOffset, to[2] ) );
        return closed;
    }

    template<typename Patch>
    auto stitch( const std::vector<Stretch>& stretches, const Patch& patch ) const { return bz2gpu::stitchFields( stretches, field, patch ); }

    static std::array<uint64_t, COLUMNS> words( const bz2gpu::FieldSpan& span ) { return { span.start, (uint64_t)span.size, 0 }; }
    static const bz2gpu::FieldSpan& tail( const bz2gpu::StitchedFields& stitched ) { return stitched.tail; }
};

/* ------------------------------------------------------------------------------------------------ the reader */
class StreamReader
{
public:
    /* parallelization 0: a batch of this many blocks keeps the GPU busy while a single cold read still returns after
     * one small launch */
    static constexpr size_t DEFAULT_BATCH = 512;

    using Sink = std::function<void( const uint8_t*, uint64_t )>;
    using OffsetMap = std::map<size_t, size_t>;

    StreamReader( std::shared_ptr<Source> source, size_t parallelization, int device ) :
        m_source( std::move( source ) ),
        m_batch( parallelization == 0 ? DEFAULT_BATCH : parallelization ),
        m_device( device ),
        m_checkStreamCrc( parallelization == 1 )   /* the reference's serial reader checks, the parallel one does not */
    {}

    void setVerifyStreamCrc( bool enable ) { m_checkStreamCrc = enable; }
    [[nodiscard]] uint64_t streamsVerified() const { return m_streamsVerified; }

    void
    close()
    {
        dropHeldLines();
        dropHeldHashes();
        m_fields.reset();
        m_fieldColumns.reset();
        dropHeldFieldHashes();
        dropHeldFieldNumbers();
        m_fieldMatches.reset();
        m_matches.reset();
        m_setMatches.reset();
        m_scheduler.reset();
        m_finder.reset();
        m_source.reset();
    }

    [[nodiscard]] bool closed() const { return !m_source; }
    [[nodiscard]] bool eof() const { return m_atEnd; }

    /** Decoded size, once the whole file has been seen (or an index was loaded). */
    [[nodiscard]] std::optional<size_t>
    size() const
    {
        if ( !m_index.sealed() ) return std::nullopt;
        return (size_t)m_index.last().second;
    }

    [[nodiscard]] size_t
    tell() const
    {
        if ( !m_atEnd ) return m_position;
        const auto total = size();
        if ( !total ) {
            fail( MI355X_BZ2_ERR_LOGIC, "at the end of the file its size has to be known" );
        }
        return *total;
    }

    /**
     * Up to `wanted` bytes from the current position into `sink` (an empty sink discards them).  Two things can happen
     * per step: the position lies in a block the index knows -- then its run is fetched and the bytes go out; or it lies
     * behind everything indexed -- then the next block of the file is decoded and indexed, which is where decode errors,
     * end-of-stream blocks, stream CRCs and the end of the file come up.
     */
    size_t
    read( const Sink& sink, size_t wanted = std::numeric_limits<size_t>::max() )
    {
        if ( closed() ) {
            fail( MI355X_BZ2_ERR_CLOSED, "read on a closed reader" );
        }
        size_t produced = 0;
        while ( ( produced < wanted ) && !m_atEnd ) {
            const auto span = m_index.locate( m_position );
            if ( !span.covers( m_position ) ) {
                if ( !indexNextBlock() ) {
                    m_atEnd = true;
                }
                continue;
            }
            const auto run = scheduler().demand( finder().numberOf( span.bits ) );
            const auto& record = recordIn( *run, span.bits );
            if ( record.status != MI355X_BZ2_OK ) {
                fail( record.status, "block at bit offset " + std::to_string( span.bits ) );
            }
            const uint64_t inBlock = m_position - span.bytes;
            if ( inBlock >= record.byteLength ) {
                fail( MI355X_BZ2_ERR_LOGIC, "the block index promises more bytes than the block decodes to" );
            }
            const uint64_t piece = std::min<uint64_t>( record.byteLength - inBlock, wanted - produced );
            if ( sink ) {
                sink( run->bytes.get() + record.at + inBlock, piece );
            }
            produced += piece;
            m_position += piece;
        }
        return produced;
    }

    /** read( fd, buffer, n ) of the interface: to a file descriptor and / or a buffer, or nowhere
     * (BZ2ReaderInterface.hpp:35-57). */
    size_t
    read( int outputFileDescriptor, char* outputBuffer, size_t wanted )
    {
        if ( ( outputFileDescriptor < 0 ) && ( outputBuffer == nullptr ) ) {
            return read( Sink(), wanted );
        }
        uint64_t copied = 0;
        return read( [&] ( const uint8_t* bytes, uint64_t size ) {
            for ( uint64_t written = 0; ( outputFileDescriptor >= 0 ) && ( written < size ); ) {
                const auto n = ::write( outputFileDescriptor, bytes + written, (size_t)std::min<uint64_t>( size - written, 1u << 30 ) );
                if ( n > 0 ) {
                    written += (uint64_t)n;
                } else if ( !( n < 0 && errno == EINTR ) ) {
                    fail( MI355X_BZ2_ERR_IO, std::string( "write: " ) + strerror( errno ) );
                }
            }
            if ( outputBuffer != nullptr ) {
                std::memcpy( outputBuffer + copied, bytes, size );
            }
            copied += size;
        }, wanted );
    }

    /** Seeking never decodes more than it has to: inside the indexed part of the file (or anywhere once the index is
     * complete) only the position changes; a target behind the indexed part is reached by decoding forward. */
    size_t
    seek( long long offset, int whence )
    {
        if ( closed() ) {
            fail( MI355X_BZ2_ERR_CLOSED, "seek on a closed reader" );
        }
        if ( ( whence == SEEK_END ) && !m_index.sealed() ) {
            read( Sink() );      /* the size is only known at the end */
        }
        long long target = offset;
        if ( whence == SEEK_CUR ) {
            target += (long long)tell();
        } else if ( whence == SEEK_END ) {
            target += (long long)size().value();
        } else if ( whence != SEEK_SET ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "invalid seek origin" );
        }
        target = std::max( target, 0LL );
        if ( const auto total = size() ) {
            target = std::min<long long>( target, (long long)*total );
        }
        const auto goal = (size_t)target;
        const size_t here = tell();
        if ( goal == here ) {
            return here;
        }
        if ( ( goal < here ) || ( goal < m_index.frontier() ) ) {
            m_position = goal;
            m_atEnd = false;
        } else if ( m_index.sealed() ) {
            m_position = (size_t)m_index.last().second;
            m_atEnd = true;
        } else {
            m_position = (size_t)m_index.frontier();
            m_atEnd = false;
            read( Sink(), goal - m_position );
        }
        return tell();
    }

    /**
     * pread of n ranges into `dst` (mi355x_bz2_reader_read_ranges): the blocks the ranges need are decoded once, in
     * launches of at most a batch, and k_gather copies just the requested bytes.  The position, eof() and the runs of the
     * sequential reader stay as they were; ranges behind the indexed part of the file are indexed first, as a forward
     * seek would.
     */
    void
    readRanges( const uint64_t* offsets, const uint64_t* sizes, size_t n, void* dst, bool dstIsDevice, uint64_t* nRead )
    {
        if ( closed() ) {
            fail( MI355X_BZ2_ERR_CLOSED, "read_ranges on a closed reader" );
        }
        uint64_t furthest = 0;
        for ( size_t i = 0; i < n; ++i ) {
            if ( sizes[i] > 0 ) furthest = std::max( furthest, offsets[i] + std::min( sizes[i], ~uint64_t( 0 ) - offsets[i] ) );
        }
        indexUpTo( furthest );
        const auto map = knownMap();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planRanges( map, offsets, sizes, n, m_batch, packed, m_source->size() );
        } );
        if ( !plan.pieces.empty() && dst == nullptr ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "read_ranges: no destination" );
        }

        std::vector<std::vector<mi355x_bz2_gather_piece> > pieces( plan.launches.size() );
        for ( const auto& piece : plan.pieces ) {
            pieces[piece.launch].push_back( { piece.src, piece.dst, piece.size } );
        }
        runJobs( plan.launches, [&] ( size_t l ) {
            return [mine = &pieces[l], dst, dstIsDevice] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) {
                gatherPieces( ctx, *mine, dst, dstIsDevice );
            };
        } );
        std::copy( plan.nRead.begin(), plan.nRead.end(), nRead );
    }

    /* ---------------------------------------------------------------------------------------- search */
    /** Step 1 (mi355x_bz2_reader_search): the launches of bz2_search.hpp's plan, each searching its extent on the context
     * that decoded it; then the matches no launch can see (seamMatches), and both merged in file order. */
    void
    search( const uint8_t* pattern, uint32_t m, uint32_t flags, uint64_t start, uint64_t end, uint64_t limit, uint64_t* nMatches )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "search on a closed reader" );
        const bool fold = ( flags & bz2gpu::SEARCH_IGNORE_CASE ) != 0;
        if ( m == 0 || m > bz2gpu::SEARCH_PATTERN_MAX ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "search: the pattern must have 1 to 256 bytes, not " + std::to_string( m ) );
        }
        m_matches.reset();
        *nMatches = 0;
        if ( start >= end ) {
            if ( limit > 0 ) m_matches.emplace();
            return;
        }
        indexUpTo( end );
        const auto map = knownMap();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planSearch( map, start, end, m, m_batch, packed, m_source->size() );
        } );
        const size_t n = plan.launches.size();
        SearchCall call{ bz2gpu::foldedBytes( pattern, m, fold ), flags, limit, SearchProgress( n ) };
        std::vector<SearchWork> searches( n );
        for ( size_t l = 0; l < n; ++l ) {
            searches[l].call = &call;
            searches[l].index = (uint32_t)l;
            searches[l].extent = plan.extents[l];
        }
        /* the launches in front of the first one that was not started: with a limit they hold at least `limit` matches,
         * and every match that needs a byte behind them starts behind all of those (bz2_search.hpp) */
        const size_t usable = runJobs( plan.launches, [&] ( size_t l ) {
            return [work = &searches[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) { runSearchWork( ctx, *work ); };
        }, &call.progress.stop );
        const auto between = bz2gpu::seamMatches( call.pattern.data(), m, extentSeams( searches, usable, m ), fold );
        if ( limit == 0 ) {
            uint64_t total = between.size();
            for ( const auto& work : searches ) total += work.count;
            *nMatches = total;
            return;
        }
        /* extent by extent: its own matches, then those that start in it and end behind it */
        std::vector<uint64_t> merged;
        size_t seam = 0;
        for ( size_t l = 0; l < usable && merged.size() < limit; ++l ) {
            const auto& extent = searches[l].extent;
            for ( const auto position : searches[l].positions ) merged.push_back( extent.fileOffset + ( position - extent.src ) );
            for ( ; seam < between.size() && between[seam] < extent.fileOffset + extent.size; ++seam ) merged.push_back( between[seam] );
        }
        if ( merged.size() > limit ) merged.resize( (size_t)limit );
        *nMatches = merged.size();
        m_matches = std::move( merged );
    }

    /** Step 1 for a set (mi355x_bz2_reader_search_set): search with searchOutputSet per launch, seamMatchesSet for the
     * pairs no launch can see, and a merge by (position, id) that is cut to the limit afterwards. */
    void
    searchSet( const bz2gpu::PatternSet& set, uint64_t start, uint64_t end, uint64_t limit, uint64_t* nMatches, uint64_t* perPattern )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "search_set on a closed reader" );
        m_setMatches.reset();
        *nMatches = 0;
        const uint32_t k = set.count();
        if ( limit == 0 && perPattern != nullptr ) std::fill_n( perPattern, k, uint64_t( 0 ) );
        if ( start >= end ) {
            if ( limit > 0 ) m_setMatches.emplace();
            return;
        }
        indexUpTo( end );
        const auto map = knownMap();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planSearchSet( map, start, end, set, m_batch, packed, m_source->size() );
        } );
        const size_t n = plan.launches.size();
        SetSearchCall call{ &set, limit, SearchProgress( n ) };
        std::vector<SetSearchWork> searches( n );
        for ( size_t l = 0; l < n; ++l ) {
            searches[l].call = &call;
            searches[l].index = (uint32_t)l;
            searches[l].extent = plan.extents[l];
        }
        /* the launches in front of the first one that was not started: with a limit they hold at least `limit` pairs that
         * sort in front of every pair that needs a byte behind them (bz2_search.hpp) */
        const size_t usable = runJobs( plan.launches, [&] ( size_t l ) {
            return [work = &searches[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) { runSetSearchWork( ctx, *work ); };
        }, &call.progress.stop );
        const auto between = bz2gpu::seamMatchesSet( set, extentSeams( searches, usable, set.mMax ) );
        if ( limit == 0 ) {
            uint64_t total = between.size();
            for ( const auto& work : searches ) total += work.count;
            *nMatches = total;
            if ( perPattern != nullptr ) {
                for ( const auto& work : searches ) {
                    for ( uint32_t i = 0; i < k; ++i ) perPattern[i] += work.perPattern[i];
                }
                for ( const auto& pair : between ) ++perPattern[pair.second];
            }
            return;
        }
        /* the extents' pairs lie in (position, id) order one extent behind the other; the seam pairs are merged into them */
        HeldSetMatches merged;
        size_t seam = 0;
        const auto full = [&] { return merged.positions.size() >= limit; };
        const auto push = [&] ( uint64_t position, uint32_t id ) {
            merged.positions.push_back( position );
            merged.ids.push_back( id );
        };
        for ( size_t l = 0; l < usable && !full(); ++l ) {
            const auto& work = searches[l];
            for ( size_t i = 0; i < work.positions.size() && !full(); ++i ) {
                const bz2gpu::SetMatch own{ work.positions[i], work.ids[i] };
                for ( ; seam < between.size() && between[seam] < own && !full(); ++seam ) push( between[seam].first, between[seam].second );
                if ( !full() ) push( own.first, own.second );
            }
            /* a launch that held more pairs than the limit has emitted `limit` of them, and the result is full by now */
            const uint64_t extentEnd = work.extent.fileOffset + work.extent.size;
            for ( ; seam < between.size() && between[seam].first < extentEnd && !full(); ++seam ) push( between[seam].first, between[seam].second );
        }
        *nMatches = merged.positions.size();
        m_setMatches = std::move( merged );
    }

    /** Step 2 (mi355x_bz2_reader_take_set_matches): the held pairs, then none are held any more. */
    void
    takeSetMatches( uint64_t* positions, uint32_t* ids, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_set_matches on a closed reader" );
        if ( !m_setMatches ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_set_matches: no matches are held (search_set with a limit first)" );
        const auto held = std::move( *m_setMatches );
        m_setMatches.reset();
        const auto n = (size_t)std::min<uint64_t>( capacity, held.positions.size() );
        std::copy_n( held.positions.begin(), n, positions );
        std::copy_n( held.ids.begin(), n, ids );
    }

    /** Step 2 (mi355x_bz2_reader_take_matches): the held positions, then nothing is held any more. */
    void
    takeMatches( uint64_t* positions, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_matches on a closed reader" );
        if ( !m_matches ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_matches: no matches are held (search with a limit first)" );
        const auto held = std::move( *m_matches );
        m_matches.reset();
        std::copy_n( held.begin(), (size_t)std::min<uint64_t>( capacity, held.size() ), positions );
    }

    /* ---------------------------------------------------------------------------------------- line access */
    using LinePairs = std::vector<std::pair<uint64_t, uint64_t> >;

    /** The line index for `nl` as {decoded offset, delimiters in front of it} pairs (mi355x_bz2_reader_line_offsets). */
    [[nodiscard]] LinePairs
    lineOffsets( uint8_t nl )
    {
        const auto& index = lineIndex( nl );
        LinePairs pairs( index.bytes.size() );
        for ( size_t i = 0; i < pairs.size(); ++i ) pairs[i] = { index.bytes[i], index.lines[i] };
        return pairs;
    }

    void
    setLineOffsets( uint8_t nl, const uint64_t* bytes, const uint64_t* lines, size_t n )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "set_line_offsets on a closed reader" );
        if ( !m_index.sealed() ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "a line index needs the complete block map: set_block_offsets or block_offsets first" );
        }
        if ( n == 0 ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "an empty line index cannot be loaded" );
        bz2gpu::checkLineIndex( m_index.snapshot(), bytes, lines, n );   /* std::invalid_argument */
        dropHeldLines();
        m_lines = LineIndex{ nl, { bytes, bytes + n }, { lines, lines + n } };
    }

    /** s(k) for every line number given (mi355x_bz2_reader_line_starts): only blocks that hold a boundary are decoded. */
    void
    lineStarts( uint8_t nl, const uint64_t* lines, size_t n, uint64_t* byteOffsets )
    {
        const auto& index = lineIndex( nl );
        dropHeldLines();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planLines( m_index.snapshot(), index.bytes.data(), index.lines.data(), index.bytes.size(),
                                      lines, nullptr, n, /* startsOnly */ true, m_batch, packed, m_source->size() );
        } );
        std::vector<uint64_t> positions( plan.queries.size(), bz2gpu::NOT_FOUND );
        std::vector<LineWork> lineWorks;
        runLineLaunches( plan, nl, positions, lineWorks );
        for ( size_t i = 0; i < n; ++i ) {
            const auto& start = plan.starts[i];
            byteOffsets[i] = start.query == bz2gpu::NO_QUERY
                             ? start.fixed : bz2gpu::lineStartOf( plan.queries[start.query], positions[start.query] );
        }
    }

    /** L(p) for every offset given (mi355x_bz2_reader_line_numbers), the inverse of lineStarts: only blocks that hold an
     * offset which is not their first byte are decoded, and k_rank_byte counts the delimiters in front of the offsets. */
    void
    lineNumbers( uint8_t nl, const uint64_t* offsets, size_t n, uint64_t* lines )
    {
        const auto& index = lineIndex( nl );
        dropHeldLines();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planLineNumbers( m_index.snapshot(), index.bytes.data(), index.lines.data(), index.bytes.size(),
                                            offsets, n, m_batch, packed, m_source->size() );
        } );
        std::vector<uint64_t> ranks( plan.queries.size(), 0 );
        std::vector<RankWork> rankWorks( plan.launches.size() );
        for ( auto& work : rankWorks ) {
            work.nl = nl;
            work.plan = &plan;
            work.ranks = ranks.data();
        }
        /* the queries come launch by launch */
        for ( size_t q = 0; q < plan.queries.size(); ++q ) {
            auto& work = rankWorks[plan.queries[q].launch];
            if ( work.count++ == 0 ) work.first = q;
        }
        runJobs( plan.launches, [&] ( size_t l ) {
            return [work = &rankWorks[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) { runRankWork( ctx, *work ); };
        } );
        for ( size_t i = 0; i < n; ++i ) lines[i] = bz2gpu::lineNumberOf( plan.answers[i], ranks.data() );
    }

    /** Step 1 of grep (mi355x_bz2_reader_grep): the search for all matches, the lines of their first bytes, repeats
     * dropped, the first maxLines of them; then -- unless only their number is wanted -- readLineRanges with one range
     * (line, 1) per matching line, whose pieces stay held for takeLineRanges.  Matches and line ranges held by earlier
     * calls are released.  The rank pass decodes the blocks with matches a second time, the line pass a third. */
    void
    grep( const uint8_t* pattern, uint32_t m, uint32_t flags, uint8_t nl, uint64_t start, uint64_t end, uint64_t maxLines,
          bool keepOnDevice, uint64_t* nLines, uint64_t* totalBytes )
    {
        uint64_t nMatches = 0;
        search( pattern, m, flags, start, end, std::numeric_limits<uint64_t>::max(), &nMatches );
        const auto positions = std::move( *m_matches );
        m_matches.reset();
        grepPositions( positions, nl, maxLines, keepOnDevice, nLines, totalBytes );
    }

    /** mi355x_bz2_reader_grep_set: grep with the set search as its first pass.  The pairs of one position are one
     * position for the rank pass. */
    void
    grepSet( const bz2gpu::PatternSet& set, uint8_t nl, uint64_t start, uint64_t end, uint64_t maxLines, bool keepOnDevice,
             uint64_t* nLines, uint64_t* totalBytes )
    {
        uint64_t nMatches = 0;
        searchSet( set, start, end, std::numeric_limits<uint64_t>::max(), &nMatches, nullptr );
        auto positions = std::move( m_setMatches->positions );
        m_setMatches.reset();
        positions.erase( std::unique( positions.begin(), positions.end() ), positions.end() );
        grepPositions( positions, nl, maxLines, keepOnDevice, nLines, totalBytes );
    }

    /** mi355x_bz2_reader_grep_regex: grep with a DFA run as its first pass.  The launches are planSearch's over the whole
     * file; each summarises its extent (matchLinesOutput), stitchSummaries composes the summaries into one offset inside
     * every matching line, and the rank and line passes are grep's.  Only the number of lines wanted: the count of
     * witnesses is the answer, nothing is emitted or ranked. */
    void
    grepRegex( const bz2gpu::Regex& regex, uint8_t nl, uint64_t maxLines, bool keepOnDevice, uint64_t* nLines, uint64_t* totalBytes )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "grep_regex on a closed reader" );
        m_matches.reset();
        const uint64_t everything = std::numeric_limits<uint64_t>::max();
        indexUpTo( everything );
        const auto map = knownMap();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planSearch( map, 0, everything, 1, m_batch, packed, m_source->size() );
        } );
        std::vector<bz2gpu::Stretch> stretches( plan.launches.size() );
        for ( size_t l = 0; l < stretches.size(); ++l ) {
            stretches[l].fileOffset = plan.extents[l].fileOffset;
            stretches[l].size = plan.extents[l].size;
        }
        runJobs( plan.launches, [&] ( size_t l ) {
            return [&regex, nl, maxLines, extent = plan.extents[l], stretch = &stretches[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) {
                checkDevice( ctx, matchLinesOutput( ctx, { extent.src, extent.size }, regex, nl, maxLines, &stretch->summary ) );
                for ( auto& witness : stretch->summary.witnesses ) witness = extent.fileOffset + ( witness - extent.src );
            };
        } );
        if ( maxLines == 0 ) {
            dropHeldLines();
            *nLines = bz2gpu::stitchSummaries( regex, stretches, nullptr );
            *totalBytes = 0;
            return;
        }
        std::vector<uint64_t> positions;
        bz2gpu::stitchSummaries( regex, stretches, &positions );
        grepPositions( positions, nl, maxLines, keepOnDevice, nLines, totalBytes );
    }

    /** The rank and line passes of grep, from the ascending positions of the matches' first bytes. */
    void
    grepPositions( const std::vector<uint64_t>& positions, uint8_t nl, uint64_t maxLines, bool keepOnDevice, uint64_t* nLines,
                   uint64_t* totalBytes )
    {
        dropHeldLines();
        *nLines = 0;
        *totalBytes = 0;
        if ( positions.empty() ) {
            /* no match: no line index is built or asked, nothing is decoded again; empty results are held */
            if ( maxLines > 0 ) {
                HeldLines held;
                held.onDevice = keepOnDevice;
                m_held = std::move( held );
                m_grep = HeldGrep{};
            }
            return;
        }
        std::vector<uint64_t> numbers( positions.size() );
        lineNumbers( nl, positions.data(), positions.size(), numbers.data() );
        numbers.erase( std::unique( numbers.begin(), numbers.end() ), numbers.end() );
        *totalBytes = 0;
        if ( maxLines > 0 && numbers.size() > maxLines ) numbers.resize( (size_t)maxLines );
        *nLines = numbers.size();
        if ( maxLines == 0 ) return;
        HeldGrep held;
        held.sizes.assign( numbers.size(), 0 );
        const std::vector<uint64_t> ones( numbers.size(), 1 );
        readLineRanges( nl, numbers.data(), ones.data(), numbers.size(), keepOnDevice, held.sizes.data(), totalBytes );
        held.numbers = std::move( numbers );
        m_grep = std::move( held );
    }

    /** mi355x_bz2_reader_take_grep: the held line numbers and sizes; the bytes stay held for takeLineRanges. */
    void
    takeGrep( uint64_t* lineNumbers, uint64_t* byteSizes, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_grep on a closed reader" );
        if ( !m_grep || !m_held ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_grep: no lines are held (grep with max_lines > 0 first)" );
        const size_t n = (size_t)std::min<uint64_t>( capacity, m_grep->numbers.size() );
        std::copy_n( m_grep->numbers.begin(), n, lineNumbers );
        std::copy_n( m_grep->sizes.begin(), n, byteSizes );
    }

    /** Step 1 of the line ranges (mi355x_bz2_reader_read_line_ranges): decode, resolve, gather into the contexts' result
     * buffers; the pieces are held for takeLineRanges. */
    void
    readLineRanges( uint8_t nl, const uint64_t* first, const uint64_t* count, size_t n, bool keepOnDevice,
                    uint64_t* byteSizes, uint64_t* total )
    {
        const auto& index = lineIndex( nl );
        dropHeldLines();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planLines( m_index.snapshot(), index.bytes.data(), index.lines.data(), index.bytes.size(),
                                      first, count, n, /* startsOnly */ false, m_batch, packed, m_source->size() );
        } );
        std::vector<uint64_t> positions( plan.queries.size(), bz2gpu::NOT_FOUND );
        std::vector<LineWork> lineWorks;
        try {
            runLineLaunches( plan, nl, positions, lineWorks );
        } catch ( ... ) {
            dropHeldLines();
            throw;
        }
        HeldLines held;
        held.onDevice = keepOnDevice;
        held.sizes.assign( n, 0 );
        /* launch by launch: a range's segments come front to back, in launch order */
        for ( const auto& work : lineWorks ) {
            for ( const auto& piece : work.held ) {
                held.sizes[piece.range] += piece.size;
                held.pieces.push_back( piece );
            }
        }
        uint64_t sum = 0;
        for ( size_t i = 0; i < n; ++i ) {
            byteSizes[i] = held.sizes[i];
            sum += held.sizes[i];
        }
        if ( total != nullptr ) *total = sum;
        m_held = std::move( held );
    }

    /** Step 2 (mi355x_bz2_reader_take_line_ranges): the held pieces to their places in `dst`, range i behind the ranges
     * in front of it; then nothing is held any more. */
    void
    takeLineRanges( void* dst, bool dstIsDevice )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_line_ranges on a closed reader" );
        if ( !m_held ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_line_ranges: no line ranges are held (read_line_ranges first)" );
        const auto held = std::move( *m_held );
        dropHeldLines();
        if ( held.onDevice != dstIsDevice ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_line_ranges: the destination is not where read_line_ranges was told it would be" );
        }
        if ( held.pieces.empty() ) return;
        if ( dst == nullptr ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_line_ranges: no destination" );
        std::vector<uint64_t> at( held.sizes.size(), 0 );
        for ( size_t i = 1; i < at.size(); ++i ) at[i] = at[i - 1] + held.sizes[i - 1];
        std::map<mi355x_bz2_ctx*, std::vector<mi355x_bz2_gather_piece> > perContext;
        for ( const auto& piece : held.pieces ) {
            perContext[piece.ctx].push_back( { piece.offset, at[piece.range], piece.size } );
            at[piece.range] += piece.size;
        }
        for ( const auto& [ctx, pieces] : perContext ) {
            checkDevice( ctx, gatherResult( ctx, pieces.data(), (uint32_t)pieces.size(), dst, dstIsDevice ? 1 : 0 ) );
        }
    }

    /** mi355x_bz2_reader_line_hashes: lineColumns with the hashing pass (hashLinesOutput) and stitchSummaries, one column. */
    void
    lineHashes( uint8_t nl, uint64_t seed, uint64_t first, uint64_t count, bool keepOnDevice, uint64_t* nLines )
    {
        const auto& index = lineIndex( nl );
        dropHeldLines();
        dropHeldHashes();
        m_hashes = lineColumns( LineHashQuery{ nl, bz2gpu::lineHashBase( seed ) }, "line_hashes", index, first, count, keepOnDevice, nLines );
    }

    /** mi355x_bz2_reader_take_line_hashes. */
    void
    takeLineHashes( void* hashes, uint64_t capacity, bool dstIsDevice )
    {
        takeColumns( "take_line_hashes", "no hashes are held (line_hashes first)", m_hashes, { hashes }, capacity, dstIsDevice );
    }

    [[nodiscard]] const uint64_t*
    lineHashesDevice() const
    {
        return m_hashes && m_hashes->onDevice && m_hashes->n > 0 ? m_hashes->column<const uint64_t>( 0 ) : nullptr;
    }

    /** mi355x_bz2_reader_distinct_lines: lineHashes over the whole file, then bz2_distinct.hip. */
    void
    distinctLines( uint8_t nl, uint64_t seed, bool wantNumbers, uint64_t* nDistinct )
    {
        uint64_t n = 0;
        lineHashes( nl, seed, 0, std::numeric_limits<uint64_t>::max(), false, &n );
        std::vector<uint64_t> numbers;
        std::string why;
        const bool done = distinctHashes( m_device, m_hashes->column<const uint64_t>( 0 ), n, nDistinct, wantNumbers ? &numbers : nullptr, &why );
        dropHeldHashes();
        if ( !done ) fail( MI355X_BZ2_ERR_DEVICE, why );
        if ( wantNumbers ) m_distinct = std::move( numbers );
    }

    /** mi355x_bz2_reader_take_distinct_lines. */
    void
    takeDistinctLines( uint64_t* lineNumbers, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_distinct_lines on a closed reader" );
        if ( !m_distinct ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_distinct_lines: no line numbers are held (distinct_lines with want_numbers first)" );
        }
        std::copy_n( m_distinct->begin(), (size_t)std::min<uint64_t>( capacity, m_distinct->size() ), lineNumbers );
    }

    /** mi355x_bz2_reader_field_spans: lineColumns with fieldSpansOutput and stitchFields, a column of starts and one of sizes. */
    void
    fieldSpans( uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count, bool keepOnDevice, uint64_t* nLines,
                std::optional<uint8_t> quote = std::nullopt )
    {
        const auto refused = quote ? bz2gpu::quotedFieldArgumentsError( nl, dl, *quote, field ) : bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "field_spans: " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        m_fields.reset();
        if ( !quote ) {
            m_fields = lineColumns( FieldSpanQuery{ nl, dl, field }, "field_spans", index, first, count, keepOnDevice, nLines );
            return;
        }
        /* mi355x_bz2_reader_field_spans_quoted: the launches wrote contents; the patched lines are raw */
        std::vector<std::pair<uint64_t, std::array<uint64_t, 2> > > patched;
        auto held = lineColumns( QuotedFieldSpanQuery{ nl, dl, *quote, field }, "field_spans", index, first, count, keepOnDevice, nLines,
                                 &patched );
        std::vector<bz2gpu::FieldSpan> fields;
        for ( const auto& [line, words] : patched ) fields.push_back( { words[0], (int64_t)words[1] } );
        quotedContents( fields, *quote, "field_spans" );
        std::string why;
        for ( size_t i = 0; i < fields.size(); ++i ) {
            const auto words = QuotedFieldSpanQuery::words( fields[i] );
            if ( words == patched[i].second ) continue;
            for ( size_t c = 0; c < words.size(); ++c ) {
                if ( !hostToDevice( m_device, held.column<uint64_t>( c ) + patched[i].first, &words[c], sizeof( words[c] ), &why ) ) {
                    fail( MI355X_BZ2_ERR_DEVICE, "field_spans: " + why );
                }
            }
        }
        m_fields = std::move( held );
    }

    /** The raw fields `fields` of the decoded file become their contents under `quote` (bz2_fieldquote.hpp): the first and
     * last byte of each that has 2 bytes or more are fetched in one call of readRanges.  These are the lines the stitchers
     * patch -- one per launch seam, and the tail -- so the blocks that hold them are the only ones decoded again. */
    void
    quotedContents( std::vector<bz2gpu::FieldSpan>& fields, uint8_t quote, const std::string& what )
    {
        std::vector<uint64_t> offsets, sizes;
        for ( const auto& field : fields ) {
            if ( field.size < 2 ) continue;
            offsets.insert( offsets.end(), { field.start, field.start + (uint64_t)field.size - 1 } );
            sizes.insert( sizes.end(), { 1, 1 } );
        }
        if ( offsets.empty() ) return;
        std::vector<uint8_t> ends( offsets.size() );
        std::vector<uint64_t> nRead( offsets.size() );
        readRanges( offsets.data(), sizes.data(), offsets.size(), ends.data(), false, nRead.data() );
        if ( nRead != sizes ) fail( MI355X_BZ2_ERR_LOGIC, what + ": a patched field lies behind the end of the file" );
        size_t at = 0;
        for ( auto& field : fields ) {
            if ( field.size < 2 ) continue;
            field = bz2gpu::quotedFieldContent( field, ends[at], ends[at + 1], quote );
            at += 2;
        }
    }

    /** mi355x_bz2_reader_take_field_spans. */
    void
    takeFieldSpans( void* starts, void* sizes, uint64_t capacity, bool dstIsDevice )
    {
        takeColumns( "take_field_spans", "no field spans are held (field_spans first)", m_fields, { starts, sizes }, capacity, dstIsDevice );
    }

    /**
     * mi355x_bz2_reader_field_columns: the launches of lineColumns' plan, in which every stretch runs fieldSpansOutput once
     * per field while it is resident -- every needed block is decoded once, whatever the number of fields -- and packs each
     * field's bytes with gatherFieldsOutput into a buffer of that stretch's own, allocated when the stretch's total is
     * known.  Then per field: stitchFields, its patches into the sizes, the final offsets scanned on the device over the
     * patched sizes (columnOffsets), planColumnAssembly (bz2_fieldcols.hpp), and the fix-ups -- the patched lines' fields,
     * one per launch seam and the tail -- fetched by readRanges, the only second decode.  The result is held as pieces:
     * the stretches' packs and the fix-ups' bytes.  Peak device memory: the columns' bytes once, and per line and field
     * 24 bytes (start, size, offset), of which the 8 of the start are given back when the call returns.
     */
    void
    fieldColumns( uint8_t nl, uint8_t dl, const uint32_t* fields, uint32_t nFields, uint64_t first, uint64_t count, bool keepOnDevice,
                  uint64_t* nLines, uint64_t* totals, std::optional<uint8_t> quote = std::nullopt )
    {
        const std::string what = "field_columns";
        if ( nFields == 0 || nFields > bz2gpu::FIELD_COLUMNS_MAX ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, what + ": the number of fields must be 1 to " + std::to_string( bz2gpu::FIELD_COLUMNS_MAX )
                                                   + ", not " + std::to_string( nFields ) );
        }
        for ( uint32_t f = 0; f < nFields; ++f ) {
            const auto refused = quote ? bz2gpu::quotedFieldArgumentsError( nl, dl, *quote, fields[f] )
                                       : bz2gpu::fieldArgumentsError( nl, dl, fields[f] );
            if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, what + ": " + refused );
        }
        /* mi355x_bz2_reader_field_columns_quoted: the same path with the quoted pass and stitcher, and the patched lines'
         * raw fields trimmed (quotedContents) before anything is made of their sizes */
        if ( quote ) {
            const uint8_t q = *quote;
            fieldColumnsBy( [nl, dl, q] ( uint32_t field ) { return QuotedFieldSpanQuery{ nl, dl, q, field }; }, quote, what, nl, fields,
                            nFields, first, count, keepOnDevice, nLines, totals );
        } else {
            fieldColumnsBy( [nl, dl] ( uint32_t field ) { return FieldSpanQuery{ nl, dl, field }; }, quote, what, nl, fields, nFields, first,
                            count, keepOnDevice, nLines, totals );
        }
    }

    /** fieldColumns for the span query that queryOf( field ) names. */
    template<typename QueryOf>
    void
    fieldColumnsBy( const QueryOf& queryOf, std::optional<uint8_t> quote, const std::string& what, uint8_t nl, const uint32_t* fields,
                    uint32_t nFields, uint64_t first, uint64_t count, bool keepOnDevice, uint64_t* nLines, uint64_t* totals )
    {
        using Stretch = typename decltype( queryOf( 0u ) )::Stretch;
        const auto& index = lineIndex( nl );
        dropHeldLines();
        m_fieldColumns.reset();
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planLineHashes( m_index.snapshot(), index.bytes.data(), index.lines.data(), index.bytes.size(), first,
                                           count, m_batch, packed, m_source->size() );
        } );
        HeldFieldColumns held;
        held.device = m_device;
        held.onDevice = keepOnDevice;
        held.columns.resize( nFields );
        if ( plan.count == 0 ) {
            m_fieldColumns = std::move( held );
            return;
        }
        using Memory = HeldFieldColumn::Memory;
        const auto allocate = [&] ( uint64_t bytes ) {
            std::string why;
            Memory memory( deviceAllocate( m_device, bytes, &why ) );
            if ( !memory ) fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            return memory;
        };
        const size_t nStretches = plan.stretches.size();
        /* a stretch's offsets are local to it and have one more entry than it has lines: stretch k's lie k entries further
         * on than its lines, so that no two stretches share one; the final offsets overwrite them */
        std::vector<Memory> starts( nFields );
        std::vector<std::vector<Stretch> > stretches( nFields, std::vector<Stretch>( nStretches ) );
        std::vector<std::vector<bz2gpu::ColumnStretch> > packed( nFields, std::vector<bz2gpu::ColumnStretch>( nStretches ) );
        for ( uint32_t f = 0; f < nFields; ++f ) {
            starts[f] = allocate( plan.count * sizeof( uint64_t ) );
            held.columns[f].sizes = allocate( plan.count * sizeof( int64_t ) );
            held.columns[f].offsets = allocate( ( plan.count + nStretches + 1 ) * sizeof( uint64_t ) );
            held.columns[f].packs.resize( nStretches );
            for ( size_t k = 0; k < nStretches; ++k ) {
                stretches[f][k].fileOffset = plan.stretches[k].fileOffset;
                stretches[f][k].summary.size = plan.stretches[k].size;
            }
        }
        const auto places = bz2gpu::placeLineColumn( plan, index.bytes.data(), index.lines.data(), index.bytes.size() );
        runLineColumn( plan, places, [&] ( mi355x_bz2_ctx* ctx, size_t k, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place ) {
            for ( uint32_t f = 0; f < nFields; ++f ) {
                auto& column = held.columns[f];
                auto* const dStarts = static_cast<uint64_t*>( starts[f].get() ) + place.at;
                auto* const dSizes = static_cast<int64_t*>( column.sizes.get() ) + place.at;
                auto& summary = stretches[f][k].summary;
                (void)queryOf( fields[f] ).pass( ctx, piece, place, { dStarts, reinterpret_cast<uint64_t*>( dSizes ) }, stretches[f][k] );
                if ( summary.count != stretches[0][k].summary.count ) {
                    fail( MI355X_BZ2_ERR_LOGIC, what + ": the passes over one stretch count different lines" );
                }
                if ( place.take == 0 ) continue;
                auto& pack = packed[f][k];
                pack.at = place.at;
                pack.take = place.take;
                std::string why;
                checkDevice( ctx, gatherFieldsOutput( ctx, dStarts, dSizes, place.take, piece.src, piece.fileOffset,
                                                      static_cast<uint64_t*>( column.offsets.get() ) + place.at + k, [&] ( uint64_t bytes ) {
                    column.packs[k].reset( deviceAllocate( m_device, bytes, &why ) );
                    return static_cast<uint8_t*>( column.packs[k].get() );
                }, &pack.total, &pack.firstSize ) );
            }
            return stretches[0][k].summary.count;
        } );

        const uint64_t wantedClosed = plan.wantedClosed();
        uint64_t lines = 0;
        std::string why;
        std::vector<std::vector<bz2gpu::ColumnPatch> > patchesOf( nFields );
        for ( uint32_t f = 0; f < nFields; ++f ) {
            auto& patches = patchesOf[f];
            const auto stitched = queryOf( fields[f] ).stitch( stretches[f], [&] ( uint64_t k, const bz2gpu::FieldSpan& field ) {
                const uint64_t line = plan.firstClosed + k;
                if ( line >= first && line - first < wantedClosed ) patches.push_back( { line - first, field.start, field.size } );
            } );
            uint64_t n = std::min( wantedClosed, plan.firstClosed + stitched.closed - first );
            if ( plan.reachesEnd && stitched.hasTail ) patches.push_back( { n++, stitched.tail.start, stitched.tail.size } );
            if ( f > 0 && n != lines ) fail( MI355X_BZ2_ERR_LOGIC, what + ": the stitchers disagree about the lines" );
            lines = n;
        }
        if ( quote ) {
            /* the raw fields of all columns' patched lines in one call */
            std::vector<bz2gpu::FieldSpan> raw;
            for ( const auto& patches : patchesOf ) {
                for ( const auto& patch : patches ) raw.push_back( { patch.start, patch.size } );
            }
            quotedContents( raw, *quote, what );
            size_t at = 0;
            for ( auto& patches : patchesOf ) {
                for ( auto& patch : patches ) {
                    patch.start = raw[at].start;
                    patch.size = raw[at++].size;
                }
            }
        }
        for ( uint32_t f = 0; f < nFields; ++f ) {
            auto& column = held.columns[f];
            const auto& patches = patchesOf[f];
            const uint64_t n = lines;
            auto* const dSizes = static_cast<int64_t*>( column.sizes.get() );
            for ( const auto& patch : patches ) {
                if ( !hostToDevice( m_device, dSizes + patch.line, &patch.size, sizeof( patch.size ), &why ) ) fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            }
            uint64_t total = 0;
            if ( !columnOffsets( m_device, dSizes, n, static_cast<uint64_t*>( column.offsets.get() ), &total, &why ) ) {
                fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            }
            try {
                column.plan = bz2gpu::planColumnAssembly( packed[f], patches );
            } catch ( const std::invalid_argument& e ) {
                fail( MI355X_BZ2_ERR_LOGIC, what + ": " + e.what() );
            }
            if ( column.plan.size != total ) fail( MI355X_BZ2_ERR_LOGIC, what + ": the assembled column and its offsets disagree about its size" );
            totals[f] = total;
        }
        /* the fix-ups of all fields in ONE call of the reader's ranges path, back to back into one buffer: a block that
         * holds patched fields of several columns is decoded once more, not once per column */
        std::vector<uint64_t> fixOffsets, fixSizes;
        uint64_t fixed = 0;
        for ( auto& column : held.columns ) {
            column.fixedAt = fixed;
            for ( const auto& fixup : column.plan.fixups ) {
                if ( fixup.size == 0 ) continue;
                fixOffsets.push_back( fixup.fileOffset );
                fixSizes.push_back( fixup.size );
                fixed += fixup.size;
            }
        }
        if ( fixed > 0 ) {
            held.fixed = allocate( fixed );
            std::vector<uint64_t> nRead( fixSizes.size() );
            readRanges( fixOffsets.data(), fixSizes.data(), fixSizes.size(), held.fixed.get(), true, nRead.data() );
            if ( nRead != fixSizes ) fail( MI355X_BZ2_ERR_LOGIC, what + ": a patched field lies behind the end of the file" );
        }
        held.n = lines;
        *nLines = lines;
        m_fieldColumns = std::move( held );
    }

    /** mi355x_bz2_reader_take_field_column: sizes and offsets of held column `column` as they are, and its bytes assembled
     * straight into `data`, piece by piece: the library holds no second copy of a column.  Each may be null. */
    void
    takeFieldColumn( uint32_t column, void* data, void* offsets, void* sizes, bool dstIsDevice )
    {
        const std::string what = "take_field_column";
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, what + " on a closed reader" );
        if ( !m_fieldColumns ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, what + ": no field columns are held (field_columns first)" );
        const auto& held = *m_fieldColumns;
        if ( column >= held.columns.size() ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, what + ": column " + std::to_string( column ) + " of " + std::to_string( held.columns.size() ) );
        }
        const auto& from = held.columns[column];
        std::string why;
        const auto copy = [&] ( void* dst, const void* src, uint64_t bytes ) {
            if ( !deviceToHost( held.device, dst, src, bytes, dstIsDevice, &why ) ) fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
        };
        if ( sizes != nullptr ) copy( sizes, from.sizes.get(), held.n * sizeof( int64_t ) );
        if ( offsets != nullptr && held.n > 0 ) copy( offsets, from.offsets.get(), ( held.n + 1 ) * sizeof( uint64_t ) );
        if ( offsets != nullptr && held.n == 0 ) {
            const uint64_t zero = 0;
            if ( !dstIsDevice ) {
                std::memcpy( offsets, &zero, sizeof( zero ) );
            } else if ( !hostToDevice( held.device, offsets, &zero, sizeof( zero ), &why ) ) {
                fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            }
        }
        if ( data == nullptr ) return;
        auto* const to = static_cast<uint8_t*>( data );
        for ( const auto& piece : from.plan.copies ) {
            copy( to + piece.dst, static_cast<const uint8_t*>( from.packs[piece.stretch].get() ) + piece.src, piece.size );
        }
        uint64_t at = from.fixedAt;
        for ( const auto& fixup : from.plan.fixups ) {
            copy( to + fixup.dst, static_cast<const uint8_t*>( held.fixed.get() ) + at, fixup.size );
            at += fixup.size;
        }
    }

    /** mi355x_bz2_reader_field_hashes: lineColumns with fieldHashesOutput and stitchFieldHashes, a column of keys in front of
     * the two of the spans.  `what` names the call in its messages: field_groups goes through here. */
    void
    fieldHashes( uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first, uint64_t count, bool keepOnDevice,
                 uint64_t* nLines, const char* what = "field_hashes" )
    {
        const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        dropHeldFieldHashes();
        m_fieldHashes = lineColumns( FieldHashQuery{ nl, dl, field, bz2gpu::lineHashBase( seed ) }, what, index, first, count,
                                     keepOnDevice, nLines );
    }

    /** mi355x_bz2_reader_take_field_hashes: the keys; the spans beside them are field_groups'. */
    void
    takeFieldHashes( void* keys, uint64_t capacity, bool dstIsDevice )
    {
        takeColumns( "take_field_hashes", "no field hashes are held (field_hashes first)", m_fieldHashes, { keys }, capacity, dstIsDevice );
    }

    /** mi355x_bz2_reader_field_groups: fieldHashes over the range, then bz2_distinct.hip's groupHashes. */
    void
    fieldGroups( uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first, uint64_t count, uint64_t* nGroups,
                 uint64_t* nMissing )
    {
        uint64_t n = 0;
        fieldHashes( nl, dl, field, seed, first, count, false, &n, "field_groups" );
        std::vector<FieldGroup> groups;
        std::string why;
        const auto& held = *m_fieldHashes;
        const bool done = groupHashes( m_device, held.column<const uint64_t>( 0 ), held.column<const uint64_t>( 1 ),
                                       held.column<const int64_t>( 2 ), n, bz2gpu::FIELD_MISSING, &groups, nMissing, &why );
        dropHeldFieldHashes();
        if ( !done ) fail( MI355X_BZ2_ERR_DEVICE, why );
        for ( auto& group : groups ) group.line += first;
        *nGroups = groups.size();
        m_fieldGroups = std::move( groups );
    }

    /** mi355x_bz2_reader_take_field_groups. */
    void
    takeFieldGroups( uint64_t* lines, uint64_t* counts, uint64_t* starts, int64_t* sizes, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_field_groups on a closed reader" );
        if ( !m_fieldGroups ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_field_groups: no groups are held (field_groups first)" );
        const size_t n = (size_t)std::min<uint64_t>( capacity, m_fieldGroups->size() );
        for ( size_t i = 0; i < n; ++i ) {
            const auto& group = ( *m_fieldGroups )[i];
            if ( lines != nullptr ) lines[i] = group.line;
            if ( counts != nullptr ) counts[i] = group.count;
            if ( starts != nullptr ) starts[i] = group.start;
            if ( sizes != nullptr ) sizes[i] = group.size;
        }
    }

    /** mi355x_bz2_reader_field_numbers: lineColumns with fieldNumbersOutput and stitchFieldNumbers, a column of numbers in
     * front of the two of the spans. */
    void
    fieldNumbers( uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count, bool keepOnDevice, uint64_t* nLines )
    {
        const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "field_numbers: " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        dropHeldFieldNumbers();
        m_fieldNumbers = lineColumns( FieldNumberQuery{ nl, dl, field }, "field_numbers", index, first, count, keepOnDevice, nLines );
    }

    /** mi355x_bz2_reader_take_field_numbers: the numbers. */
    void
    takeFieldNumbers( void* numbers, uint64_t capacity, bool dstIsDevice )
    {
        takeColumns( "take_field_numbers", "no field numbers are held (field_numbers first)", m_fieldNumbers, { numbers }, capacity,
                     dstIsDevice );
    }

    /** mi355x_bz2_reader_field_sums: lineColumns with both passes per stretch (FieldSumQuery), then bz2_distinct.hip's
     * groupSums over the four columns. */
    void
    fieldSums( uint8_t nl, uint8_t dl, uint32_t keyField, uint32_t valueField, uint64_t seed, uint64_t first, uint64_t count,
               uint64_t* nGroups, uint64_t* nMissing )
    {
        for ( const auto field : { keyField, valueField } ) {
            const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
            if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "field_sums: " + refused );
        }
        const auto& index = lineIndex( nl );
        dropHeldLines();
        dropHeldFieldNumbers();
        uint64_t n = 0;
        const auto held = lineColumns( FieldSumQuery{ nl, dl, keyField, valueField, bz2gpu::lineHashBase( seed ) }, "field_sums", index,
                                       first, count, false, &n );
        std::vector<FieldSumGroup> groups;
        std::string why;
        if ( !groupSums( m_device, held.column<const uint64_t>( 0 ), held.column<const uint64_t>( 1 ), held.column<const int64_t>( 2 ),
                         held.column<const int64_t>( 3 ), n, bz2gpu::FIELD_MISSING, &groups, nMissing, &why ) ) {
            fail( MI355X_BZ2_ERR_DEVICE, why );
        }
        for ( auto& group : groups ) group.line += first;
        *nGroups = groups.size();
        m_fieldSums = std::move( groups );
    }

    /** mi355x_bz2_reader_take_field_sums. */
    void
    takeFieldSums( uint64_t* lines, uint64_t* counts, uint64_t* starts, int64_t* sizes, uint64_t* numbers, uint64_t* sumsLo,
                   int64_t* sumsHi, int64_t* mins, int64_t* maxs, uint64_t capacity )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_field_sums on a closed reader" );
        if ( !m_fieldSums ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_field_sums: no sums are held (field_sums first)" );
        const size_t n = (size_t)std::min<uint64_t>( capacity, m_fieldSums->size() );
        for ( size_t i = 0; i < n; ++i ) {
            const auto& group = ( *m_fieldSums )[i];
            if ( lines != nullptr ) lines[i] = group.line;
            if ( counts != nullptr ) counts[i] = group.count;
            if ( starts != nullptr ) starts[i] = group.start;
            if ( sizes != nullptr ) sizes[i] = group.size;
            if ( numbers != nullptr ) numbers[i] = group.numbers;
            if ( sumsLo != nullptr ) sumsLo[i] = group.sumLo;
            if ( sumsHi != nullptr ) sumsHi[i] = group.sumHi;
            if ( mins != nullptr ) mins[i] = group.min;
            if ( maxs != nullptr ) maxs[i] = group.max;
        }
    }

    /** mi355x_bz2_reader_field_matches: the lines of [first, first + count) whose field is one of the table's values, or
     * with `invert` the others.  lineColumns with FieldMatchQuery: every block is decoded once, the field-hash pass and
     * k_field_match run over each resident stretch.  The lines that cross a launch seam and the unterminated tail come
     * from the stitcher as ( key, start, size ) without bytes: for those whose key and size hit the table the field's bytes
     * are fetched by ONE readRanges call -- a second decode of their blocks, at most launches + 1 of them -- and compared
     * on the host.  Then bz2_distinct.hip's selectLines over the flags; the first `limit` numbers are held. */
    void
    fieldMatches( uint8_t nl, uint8_t dl, uint32_t field, const bz2gpu::ValueTable& table, uint64_t seed, bool invert, uint64_t first,
                  uint64_t count, uint64_t limit, bool keepOnDevice, uint64_t* nSelected, uint64_t* nMatching,
                  const char* what = "field_matches" )
    {
        const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        m_fieldMatches.reset();
        uint64_t n = 0;
        std::vector<std::pair<uint64_t, std::array<uint64_t, FieldMatchQuery::COLUMNS> > > patched;
        const auto held = lineColumns( FieldMatchQuery{ nl, dl, field, bz2gpu::lineHashBase( seed ), &table }, what, index, first, count,
                                       false, &n, &patched );
        /* the seam lines and the tail: an empty field that hits is decided, the others need their bytes */
        std::vector<uint64_t> hits, at, offsets, sizes;
        std::vector<uint32_t> values;
        uint64_t bytes = 0;
        for ( const auto& [line, words] : patched ) {
            const uint32_t value = table.candidateValue( words[0], (int64_t)words[2] );
            if ( value == table.count() ) continue;
            if ( words[2] == 0 ) {
                hits.push_back( line );
                continue;
            }
            at.push_back( line );
            values.push_back( value );
            offsets.push_back( words[1] );
            sizes.push_back( words[2] );
            bytes += words[2];
        }
        if ( !at.empty() ) {
            std::vector<uint8_t> fetched( (size_t)bytes );
            std::vector<uint64_t> nRead( at.size() );
            readRanges( offsets.data(), sizes.data(), at.size(), fetched.data(), false, nRead.data() );
            if ( nRead != sizes ) fail( MI355X_BZ2_ERR_LOGIC, std::string( what ) + ": a patched field lies behind the end of the file" );
            uint64_t from = 0;
            for ( size_t i = 0; i < at.size(); ++i ) {
                if ( std::memcmp( table.values[values[i]].data(), fetched.data() + from, (size_t)sizes[i] ) == 0 ) hits.push_back( at[i] );
                from += sizes[i];
            }
        }
        std::string why;
        const uint64_t one = 1;
        for ( const auto line : hits ) {
            if ( !hostToDevice( m_device, held.column<uint64_t>( 3 ) + line, &one, sizeof( one ), &why ) ) {
                fail( MI355X_BZ2_ERR_DEVICE, std::string( what ) + ": " + why );
            }
        }
        LinePredicate predicate;
        predicate.dFlags = held.column<const uint64_t>( 3 );
        predicate.invert = invert;
        holdSelectedLines( what, predicate, n, first, limit, keepOnDevice, nSelected, nMatching );
    }

    /** mi355x_bz2_reader_field_in_range: the lines whose field is a number n with lo <= n <= hi, or with `invert` the
     * others.  FieldNumberQuery as field_numbers runs it, then selectLines over its number column: a range needs no
     * bytes. */
    void
    fieldInRange( uint8_t nl, uint8_t dl, uint32_t field, const bz2gpu::NumberRange& range, bool invert, uint64_t first, uint64_t count,
                  uint64_t limit, bool keepOnDevice, uint64_t* nSelected, uint64_t* nMatching, const char* what = "field_in_range" )
    {
        const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        m_fieldMatches.reset();
        uint64_t n = 0;
        const auto held = lineColumns( FieldNumberQuery{ nl, dl, field }, what, index, first, count, false, &n );
        LinePredicate predicate;
        predicate.dNumbers = held.column<const int64_t>( 0 );
        predicate.lo = range.lo;
        predicate.hi = range.hi;
        predicate.invert = invert;
        holdSelectedLines( what, predicate, n, first, limit, keepOnDevice, nSelected, nMatching );
    }

    /** mi355x_bz2_reader_field_matches_regex: the lines of [first, first + count) whose field matches the automaton
     * (bz2_fieldregex.hpp), or with `invert` the others.  lineColumns with FieldRegexQuery: every block is decoded once, the
     * field-span pass and k_field_regex run over each resident stretch.  The lines that cross a launch seam and the
     * unterminated tail come from the stitcher as ( start, size ) without bytes: an empty field is decided by
     * acceptsAtEnd[0], the bytes of the others are fetched by ONE readRanges call -- a second decode of their blocks, at
     * most launches + 1 of them -- and decided by fieldRegexHolds on the host.  Then bz2_distinct.hip's selectLines over the
     * flags; the first `limit` numbers are held. */
    void
    fieldMatchesRegex( uint8_t nl, uint8_t dl, uint32_t field, const bz2gpu::Regex& regex, bool invert, uint64_t first, uint64_t count,
                       uint64_t limit, bool keepOnDevice, uint64_t* nSelected, uint64_t* nMatching,
                       const char* what = "field_matches_regex" )
    {
        const auto refused = bz2gpu::fieldArgumentsError( nl, dl, field );
        if ( !refused.empty() ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": " + refused );
        const auto& index = lineIndex( nl );
        dropHeldLines();
        m_fieldMatches.reset();
        uint64_t n = 0;
        std::vector<std::pair<uint64_t, std::array<uint64_t, FieldRegexQuery::COLUMNS> > > patched;
        const auto held = lineColumns( FieldRegexQuery{ nl, dl, field, &regex }, what, index, first, count, false, &n, &patched );
        std::vector<uint64_t> hits, at, offsets, sizes;
        uint64_t bytes = 0;
        for ( const auto& [line, words] : patched ) {
            const auto size = (int64_t)words[1];
            if ( size < 0 ) continue;
            if ( size == 0 ) {
                if ( regex.acceptsAtEnd[bz2gpu::REGEX_START] != 0 ) hits.push_back( line );
                continue;
            }
            at.push_back( line );
            offsets.push_back( words[0] );
            sizes.push_back( words[1] );
            bytes += words[1];
        }
        if ( !at.empty() ) {
            std::vector<uint8_t> fetched( (size_t)bytes );
            std::vector<uint64_t> nRead( at.size() );
            readRanges( offsets.data(), sizes.data(), at.size(), fetched.data(), false, nRead.data() );
            if ( nRead != sizes ) fail( MI355X_BZ2_ERR_LOGIC, std::string( what ) + ": a patched field lies behind the end of the file" );
            uint64_t from = 0;
            for ( size_t i = 0; i < at.size(); ++i ) {
                if ( bz2gpu::fieldRegexHolds( regex, fetched.data() + from, (int64_t)sizes[i] ) ) hits.push_back( at[i] );
                from += sizes[i];
            }
        }
        std::string why;
        const uint64_t one = 1;
        for ( const auto line : hits ) {
            if ( !hostToDevice( m_device, held.column<uint64_t>( 2 ) + line, &one, sizeof( one ), &why ) ) {
                fail( MI355X_BZ2_ERR_DEVICE, std::string( what ) + ": " + why );
            }
        }
        LinePredicate predicate;
        predicate.dFlags = held.column<const uint64_t>( 2 );
        predicate.invert = invert;
        holdSelectedLines( what, predicate, n, first, limit, keepOnDevice, nSelected, nMatching );
    }

    /** mi355x_bz2_reader_take_field_matches: the first min( capacity, held ) line numbers; they stay held. */
    void
    takeFieldMatches( void* numbers, uint64_t capacity, bool dstIsDevice )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "take_field_matches on a closed reader" );
        if ( !m_fieldMatches ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "take_field_matches: no line numbers are held (field_matches or field_in_range first)" );
        }
        std::string why;
        if ( !deviceToHost( m_fieldMatches->device, numbers, m_fieldMatches->numbers.get(), std::min( capacity, m_fieldMatches->n ) * 8,
                            dstIsDevice, &why ) ) {
            fail( MI355X_BZ2_ERR_DEVICE, "take_field_matches: " + why );
        }
    }

    /** mi355x_bz2_reader_select_lines: the selection (select( limit, &nSelected, &nMatching ) is fieldMatches or
     * fieldInRange with everything else bound), then -- unless only the number of lines is wanted -- readLineRanges with
     * one range ( line, 1 ) per selected line, exactly as grepPositions hands them over: the result is held as grep's. */
    template<typename Select>
    void
    selectLines( const Select& select, uint8_t nl, uint64_t maxLines, bool keepOnDevice, uint64_t* nLines, uint64_t* totalBytes )
    {
        uint64_t nSelected = 0, nMatching = 0;
        select( maxLines, &nSelected, &nMatching );
        *totalBytes = 0;
        *nLines = maxLines == 0 ? nMatching : nSelected;
        if ( maxLines == 0 ) {
            m_fieldMatches.reset();
            return;
        }
        std::vector<uint64_t> numbers( (size_t)nSelected );
        takeFieldMatches( numbers.data(), nSelected, false );
        m_fieldMatches.reset();
        if ( numbers.empty() ) {
            HeldLines held;
            held.onDevice = keepOnDevice;
            m_held = std::move( held );
            m_grep = HeldGrep{};
            return;
        }
        HeldGrep held;
        held.sizes.assign( numbers.size(), 0 );
        const std::vector<uint64_t> ones( numbers.size(), 1 );
        readLineRanges( nl, numbers.data(), ones.data(), numbers.size(), keepOnDevice, held.sizes.data(), totalBytes );
        held.numbers = std::move( numbers );
        m_grep = std::move( held );
    }

    [[nodiscard]] bool indexComplete() const { return m_index.sealed(); }

    [[nodiscard]] OffsetMap
    blockOffsets()
    {
        if ( !m_index.sealed() ) {
            read( Sink() );
            if ( !m_index.sealed() || !finder().complete() ) {
                fail( MI355X_BZ2_ERR_LOGIC, "the whole file was read but its block index is not complete" );
            }
        }
        return availableBlockOffsets();
    }

    [[nodiscard]] OffsetMap
    availableBlockOffsets() const
    {
        const auto pairs = m_index.snapshot();
        return { pairs.begin(), pairs.end() };
    }

    /** Import of a complete index: at least one block and the end-of-file entry.  Entries followed by an equal decoded
     * offset are end-of-stream blocks and are not handed to the finder (ParallelBZ2Reader.hpp:365-378, 456-475). */
    void
    setBlockOffsets( const OffsetMap& offsets )
    {
        if ( offsets.empty() ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "an empty index cannot be loaded: open a new reader instead" );
        }
        handOffsetsToFinder( offsets );
        if ( offsets.size() < 2 ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "an index needs at least one block and the end-of-file entry" );
        }
        m_index.assign( BlockIndex::Pairs( offsets.begin(), offsets.end() ) );
        m_lines.reset();   /* a line index belongs to the block map it was built or checked against */
    }

    [[nodiscard]] size_t
    tellCompressed() const
    {
        const auto span = m_index.locate( m_position );
        if ( span.covers( m_position ) ) return (size_t)span.bits;
        return m_index.empty() ? 0 : (size_t)m_index.last().first;
    }

    void
    joinThreads()
    {
        dropHeldLines();   /* they live in the contexts' buffers */
        m_scheduler.reset();
        m_finder.reset();
    }

    [[nodiscard]] mi355x_bz2_reader_stats
    statistics() const
    {
        return m_scheduler ? m_scheduler->statistics() : mi355x_bz2_reader_stats{};
    }

private:
    struct LineIndex
    {
        uint8_t nl{ 0 };
        std::vector<uint64_t> bytes, lines;   /* one entry per data block and the end */
    };

    struct HeldLines
    {
        bool onDevice{ false };
        std::vector<uint64_t> sizes;                       /* per range */
        std::vector<HeldPiece> pieces;                     /* front to back within every range */
    };

    struct HeldGrep
    {
        std::vector<uint64_t> numbers, sizes;              /* per matching line; the bytes are m_held's */
    };

    /** The result of a per-line column query, in device memory of the reader's own: up to four columns of n 8-byte words
     * -- hashes; starts and sizes; keys, starts and sizes; numbers, starts and sizes; keys, starts, sizes and values; keys,
     * starts, sizes and flags; starts, sizes and flags.  An empty result has no memory. */
    struct HeldColumns
    {
        struct Release { void operator()( void* pointer ) const { deviceRelease( pointer ); } };
        std::array<std::unique_ptr<void, Release>, 4> columns;
        uint64_t n{ 0 };
        int device{ -1 };
        bool onDevice{ false };

        template<typename T>
        [[nodiscard]] T* column( size_t c ) const { return static_cast<T*>( columns[c].get() ); }
    };

    /** One column of field_columns, held as pieces: sizes (n int64) and offsets (n + 1 uint64) as they are, the bytes as
     * the packs of the plan's stretches (null where a stretch packed nothing) and the fix-ups' bytes, back to back in the
     * assembly's order in the buffer all columns share; `plan` says where each piece goes. */
    struct HeldFieldColumn
    {
        using Memory = std::unique_ptr<void, HeldColumns::Release>;
        Memory sizes, offsets;
        std::vector<Memory> packs;
        bz2gpu::ColumnAssembly plan;
        uint64_t fixedAt{ 0 };                  /* where its fix-ups begin in HeldFieldColumns::fixed */
    };

    struct HeldFieldColumns
    {
        std::vector<HeldFieldColumn> columns;
        HeldFieldColumn::Memory fixed;          /* the fix-ups' bytes of all columns, column by column */
        uint64_t n{ 0 };
        int device{ -1 };
        bool onDevice{ false };
    };

    /** The line numbers field_matches and field_in_range select, in device memory of the reader's own. */
    struct HeldFieldMatches
    {
        std::unique_ptr<void, HeldColumns::Release> numbers;
        uint64_t n{ 0 };
        int device{ -1 };
        bool onDevice{ false };
    };

    /** selectLines over the n lines of a finished column, numbered from `first`: the first `limit` numbers are held. */
    void
    holdSelectedLines( const char* what, const LinePredicate& predicate, uint64_t n, uint64_t first, uint64_t limit, bool keepOnDevice,
                       uint64_t* nSelected, uint64_t* nMatching )
    {
        std::string why;
        uint64_t* selected = nullptr;
        if ( !mi355x::selectLines( m_device, predicate, n, first, limit, &selected, nMatching, &why ) ) {
            fail( MI355X_BZ2_ERR_DEVICE, std::string( what ) + ": " + why );
        }
        HeldFieldMatches held;
        held.numbers.reset( selected );
        held.n = std::min( *nMatching, limit );
        held.device = m_device;
        held.onDevice = keepOnDevice;
        *nSelected = held.n;
        m_fieldMatches = std::move( held );
    }

    void
    dropHeldFieldHashes()
    {
        m_fieldHashes.reset();
        m_fieldGroups.reset();
    }

    void
    dropHeldFieldNumbers()
    {
        m_fieldNumbers.reset();
        m_fieldSums.reset();
    }

    void
    dropHeldHashes()
    {
        m_hashes.reset();
        m_distinct.reset();
    }

    void
    dropHeldLines()
    {
        m_held.reset();
        m_grep.reset();
        const std::scoped_lock lock( m_heldBytes.mutex );
        m_heldBytes.of.clear();   /* the buffers stay: they only grow */
    }

    /** read( nowhere, wanted ) from the end of the indexed part of the file, as a forward seek would; the position and
     * eof() stay as they are, also when the read fails. */
    void
    indexForward( size_t wanted = std::numeric_limits<size_t>::max() )
    {
        const size_t position = std::exchange( m_position, (size_t)m_index.frontier() );
        const bool atEnd = std::exchange( m_atEnd, false );
        try {
            read( Sink(), wanted );
        } catch ( ... ) {
            m_position = position;
            m_atEnd = atEnd;
            throw;
        }
        m_position = position;
        m_atEnd = atEnd;
    }

    /** Index the file up to the decoded offset `furthest`. */
    void
    indexUpTo( uint64_t furthest )
    {
        if ( m_index.sealed() || ( furthest <= m_index.frontier() ) ) return;
        indexForward( (size_t)( furthest - m_index.frontier() ) );
    }

    /** The map as far as it is known; while it is not complete, its last entry is followed by the end of the open block. */
    [[nodiscard]] std::vector<std::pair<uint64_t, uint64_t> >
    knownMap() const
    {
        auto map = m_index.snapshot();
        if ( !m_index.sealed() && !map.empty() ) {
            const auto open = m_index.locate( map.back().second );
            if ( open.bitLength > 0 ) map.emplace_back( map.back().first + open.bitLength, map.back().second + open.byteLength );
        }
        return map;
    }

    /** make( packed ) plans a call's launches; packed: the compressed file is not resident on the GPU and every launch
     * brings the packed windows of its own blocks (bz2_ranges.hpp).  Only the scheduler knows which it is, and a plan
     * without launches must not create one (and with it a GPU context): while there is none yet, the plan is made as
     * for a resident file and made again if it has launches and their scheduler says otherwise. */
    template<typename MakePlan>
    [[nodiscard]] auto
    planLaunches( const MakePlan& make ) -> decltype( make( false ) )
    {
        auto plan = make( m_scheduler && !m_scheduler->inputResident() );
        if ( !m_scheduler && !plan.launches.empty() && !scheduler().inputResident() ) plan = make( true );
        return plan;
    }

    /** One job per launch of a plan, with afterDecodeOf( l ) as the job of launch l and `cancel`, if given, as the flag
     * that keeps jobs not yet taken from being started.  Each job goes to the front of the queue -- the last one first,
     * so that the first launch is taken first.  ALL of them are waited for before this returns or throws: that is what
     * allows a job to point into the caller's plan, results and destination.  Then the first failure in launch order
     * is thrown; otherwise the number of launches in front of the first cancelled one comes back. */
    size_t
    runJobs( const std::vector<bz2gpu::RangeLaunch>& launches,
             const std::function<BatchScheduler::Job::AfterDecode( size_t )>& afterDecodeOf,
             const std::atomic<bool>* cancel = nullptr )
    {
        std::vector<std::future<bool> > pending( launches.size() );
        for ( size_t l = launches.size(); l-- > 0; ) {
            auto job = std::make_unique<BatchScheduler::Job>();
            job->launch = &launches[l];
            job->cancel = cancel;
            job->afterDecode = afterDecodeOf( l );
            pending[l] = scheduler().submit( std::move( job ) );
        }
        std::exception_ptr failure;
        size_t started = pending.size();
        for ( size_t l = 0; l < pending.size(); ++l ) {
            try {
                if ( !pending[l].get() ) started = std::min( started, l );
            } catch ( ... ) {
                if ( !failure ) failure = std::current_exception();
            }
        }
        if ( failure ) std::rethrow_exception( failure );
        return started;
    }

    /** The launches of a line plan, each with its own queries and segments. */
    void
    runLineLaunches( const bz2gpu::LinePlan& plan, uint8_t nl, std::vector<uint64_t>& positions, std::vector<LineWork>& lineWorks )
    {
        lineWorks.assign( plan.launches.size(), {} );
        for ( auto& work : lineWorks ) {
            work.nl = nl;
            work.plan = &plan;
            work.positions = positions.data();
        }
        for ( size_t q = 0; q < plan.queries.size(); ++q ) lineWorks[plan.queries[q].launch].queries.push_back( (uint32_t)q );
        for ( size_t k = 0; k < plan.segments.size(); ++k ) lineWorks[plan.segments[k].launch].segments.push_back( (uint32_t)k );
        runLineJobs( plan.launches, lineWorks );
    }

    /** Launch l as a job that does lineWorks[l]. */
    void
    runLineJobs( const std::vector<bz2gpu::RangeLaunch>& launches, std::vector<LineWork>& lineWorks )
    {
        runJobs( launches, [&] ( size_t l ) {
            return [this, work = &lineWorks[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& launch ) {
                runLineWork( ctx, launch, *work, m_heldBytes );
            };
        } );
    }

    /** The launches of `plan`, in which perStretch( ctx, k, stretch, place ) does stretch k on the context that decoded it
     * and returns the number of lines it found the stretch to close, which has to be the index's (places[k].closed). */
    template<typename PerStretch>
    void
    runLineColumn( const bz2gpu::LineHashPlan& plan, const std::vector<bz2gpu::ColumnPlace>& places, const PerStretch& perStretch )
    {
        std::vector<std::vector<size_t> > ofLaunch( plan.launches.size() );
        for ( size_t k = 0; k < plan.stretches.size(); ++k ) ofLaunch[plan.stretches[k].launch].push_back( k );
        runJobs( plan.launches, [&] ( size_t l ) {
            return [&plan, &places, &perStretch, mine = &ofLaunch[l]] ( mi355x_bz2_ctx* ctx, const bz2gpu::RangeLaunch& ) {
                for ( const auto k : *mine ) {
                    const auto& piece = plan.stretches[k];
                    const uint64_t counted = perStretch( ctx, k, piece, places[k] );
                    if ( counted != places[k].closed ) failLyingLineIndex( piece.fileOffset, places[k].closed, counted );
                }
            };
        } );
    }

    /** What line_hashes, field_spans, field_hashes, field_numbers, field_sums, field_matches and field_matches_regex do, given the `query` (the
     * structs in front of the reader):
     * the launches of planLineHashes for lines [first, first + count), each doing its stretches on the context that
     * decoded them, straight into device columns that are allocated before anything is launched and in which every
     * stretch knows its place (placeLineColumn); then the query's stitcher over the stretches' summaries, and one 8-byte
     * copy per column for every line that crosses a seam and for the unterminated tail (*patched, if wanted, receives
     * those lines and their words).  *nLines = the lines of the result, which the caller holds.  A range without lines gives a result without memory.  `what` starts the messages. */
    template<typename Query>
    [[nodiscard]] HeldColumns
    lineColumns( const Query& query, const std::string& what, const LineIndex& index, uint64_t first, uint64_t count,
                 bool keepOnDevice, uint64_t* nLines,
                 std::vector<std::pair<uint64_t, std::array<uint64_t, Query::COLUMNS> > >* patched = nullptr )
    {
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planLineHashes( m_index.snapshot(), index.bytes.data(), index.lines.data(), index.bytes.size(), first,
                                           count, m_batch, packed, m_source->size() );
        } );
        *nLines = 0;
        HeldColumns held;
        held.onDevice = keepOnDevice;
        if ( plan.count == 0 ) return held;
        std::vector<typename Query::Stretch> stretches( plan.stretches.size() );
        for ( size_t k = 0; k < stretches.size(); ++k ) {
            stretches[k].fileOffset = plan.stretches[k].fileOffset;
            Query::size( stretches[k] ) = plan.stretches[k].size;
        }
        std::string why;
        held.device = m_device;
        std::array<uint64_t*, Query::COLUMNS> columns{};
        for ( size_t c = 0; c < columns.size(); ++c ) {
            held.columns[c].reset( deviceAllocate( m_device, plan.count * sizeof( uint64_t ), &why ) );
            if ( !held.columns[c] ) fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            columns[c] = held.column<uint64_t>( c );
        }
        const auto places = bz2gpu::placeLineColumn( plan, index.bytes.data(), index.lines.data(), index.bytes.size() );
        runLineColumn( plan, places, [&] ( mi355x_bz2_ctx* ctx, size_t k, const ColumnPiece& piece, const bz2gpu::ColumnPlace& place ) {
            auto to = columns;
            for ( auto& column : to ) column += place.at;
            return query.pass( ctx, piece, place, to, stretches[k] );
        } );
        /* the first closed line of a stretch is line firstClosed + k of the file */
        const uint64_t wantedClosed = plan.wantedClosed();
        std::vector<std::pair<uint64_t, std::array<uint64_t, Query::COLUMNS> > > patches;
        const auto stitched = query.stitch( stretches, [&] ( uint64_t k, const auto& value ) {
            const uint64_t line = plan.firstClosed + k;
            if ( line >= first && line - first < wantedClosed ) patches.emplace_back( line - first, Query::words( value ) );
        } );
        uint64_t n = std::min( wantedClosed, plan.firstClosed + stitched.closed - first );
        if ( plan.reachesEnd && stitched.hasTail ) patches.emplace_back( n++, Query::words( Query::tail( stitched ) ) );
        for ( const auto& [at, words] : patches ) {
            for ( size_t c = 0; c < columns.size(); ++c ) {
                if ( !hostToDevice( m_device, columns[c] + at, &words[c], sizeof( words[c] ), &why ) ) fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            }
        }
        held.n = n;
        *nLines = n;
        if ( patched != nullptr ) *patched = std::move( patches );
        return held;
    }

    /** What the takes of the column queries do: the first min( capacity, n ) words of the first columns of `held` to the
     * destinations `to`, one per column; the result stays held. */
    void
    takeColumns( const std::string& what, const char* nothingHeld, const std::optional<HeldColumns>& held,
                 std::initializer_list<void*> to, uint64_t capacity, bool dstIsDevice )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, what + " on a closed reader" );
        if ( !held ) fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, what + ": " + nothingHeld );
        std::string why;
        size_t c = 0;
        for ( void* const destination : to ) {
            if ( !deviceToHost( held->device, destination, held->columns[c++].get(), std::min( capacity, held->n ) * sizeof( uint64_t ),
                                dstIsDevice, &why ) ) {
                fail( MI355X_BZ2_ERR_DEVICE, what + ": " + why );
            }
        }
    }

    /** The line index for `nl`: the one the reader holds, or a new one.  The block map is completed first if it has to
     * be (the position and eof() stay); then every data block is decoded once more, in launches of the read_ranges kind
     * that count `nl` per block and copy nothing out. */
    [[nodiscard]] const LineIndex&
    lineIndex( uint8_t nl )
    {
        if ( closed() ) fail( MI355X_BZ2_ERR_CLOSED, "line access on a closed reader" );
        if ( m_lines && m_lines->nl == nl ) return *m_lines;
        dropHeldLines();
        if ( !m_index.sealed() ) {
            indexForward();
            if ( !m_index.sealed() ) fail( MI355X_BZ2_ERR_LOGIC, "the whole file was read but its block index is not complete" );
        }
        const auto map = m_index.snapshot();
        const uint64_t total = map.empty() ? 0 : map.back().second;
        const uint64_t offset = 0;
        const auto plan = planLaunches( [&] ( bool packed ) {
            return bz2gpu::planRanges( map, &offset, &total, 1, m_batch, packed, m_source->size() );
        } );
        std::vector<LineWork> lineWorks( plan.launches.size() );
        for ( auto& work : lineWorks ) {
            work.nl = nl;
            work.countBlocks = true;
        }
        runLineJobs( plan.launches, lineWorks );
        LineIndex index;
        index.nl = nl;
        std::vector<uint64_t> lengths;
        bz2gpu::dataBlocksOf( map, index.bytes, lengths );
        index.bytes.push_back( total );
        index.lines.push_back( 0 );
        for ( const auto& work : lineWorks ) {
            for ( const auto count : work.blockCounts ) index.lines.push_back( index.lines.back() + count );
        }
        if ( index.lines.size() != index.bytes.size() ) fail( MI355X_BZ2_ERR_LOGIC, "the line index does not match the block map" );
        m_lines = std::move( index );
        return *m_lines;
    }

    [[nodiscard]] static const BlockRecord&
    recordIn( const DecodedRun& run, uint64_t bits )
    {
        const auto record = std::lower_bound( run.blocks.begin(), run.blocks.end(), bits,
                                              [] ( const BlockRecord& r, uint64_t b ) { return r.bits < b; } );
        if ( ( record == run.blocks.end() ) || ( record->bits != bits ) ) {
            fail( MI355X_BZ2_ERR_LOGIC, "the decoded run does not hold the block it was fetched for" );
        }
        return *record;
    }

    /**
     * Decodes the first block the index does not know yet and appends it -- together with the end-of-stream block behind
     * it, if there is one (those have a magic of their own and are not in the finder's list).  False at the end of the
     * file, where the index is sealed.  The stream CRC is folded over the blocks in this order (BZ2Reader.hpp:481-484).
     */
    bool
    indexNextBlock()
    {
        const size_t number = m_index.dataBlocks();
        const auto bits = finder().at( number ).bits;
        if ( !bits ) {
            m_index.seal();
            return false;
        }
        const auto run = scheduler().demand( number );
        const auto& block = run->at( number );
        if ( block.status != MI355X_BZ2_OK ) {
            fail( block.status, "block at bit offset " + std::to_string( *bits ) );
        }
        m_index.append( block.bits, block.bitLength, block.byteLength );
        m_streamCrc = ( ( m_streamCrc << 1U ) | ( m_streamCrc >> 31U ) ) ^ block.computedCrc;
        if ( block.endOfFile ) {
            return true;
        }
        const auto next = scheduler().peekHeader( block.bits + block.bitLength );
        if ( !next.endOfStream ) {
            return true;
        }
        m_index.append( next.bits, next.bitLength, 0 );
        /* the end-of-stream block carries the CRC of the whole stream (BZ2Reader.hpp:406-416) */
        const auto folded = std::exchange( m_streamCrc, 0U );
        if ( m_checkStreamCrc ) {
            if ( next.storedCrc != folded ) {
                std::stringstream message;
                message << "stream CRC 0x" << std::hex << next.storedCrc << " in the file, 0x" << folded << " calculated";
                fail( MI355X_BZ2_ERR_STREAM_CRC, message.str() );
            }
            ++m_streamsVerified;
        }
        const uint64_t behind = next.bits + next.bitLength;
        if ( ( behind < m_source->sizeInBits() )
             && ( mi355x_bz2_read_stream_header( m_source->bytes(), m_source->size(), behind ) == 0 ) ) {
            std::cerr << "[Warning] Trailing garbage after EOF ignored!\n";
            m_finder->cut( m_index.dataBlocks() );   /* whatever the finder saw in the garbage is not a block */
        }
        return true;
    }

    BlockFinder&
    finder()
    {
        if ( !m_finder ) {
            const unsigned cores = std::max( 1u, std::thread::hardware_concurrency() );
            /* scan ahead of the decoder by a few batches (3 * hardware_concurrency blocks in the reference, BlockFinder.hpp:213) */
            m_finder = std::make_shared<BlockFinder>( m_source->bytes(), m_source->size(), MI355X_BZ2_MAGIC_BLOCK,
                                                      std::max<size_t>( 3 * cores, 4 * m_batch ),
                                                      std::min( 8u, std::max( 1u, cores / 2 ) ) );
            if ( m_index.sealed() ) {
                const auto pairs = m_index.snapshot();
                handOffsetsToFinder( OffsetMap( pairs.begin(), pairs.end() ) );
            }
        }
        return *m_finder;
    }

    BatchScheduler&
    scheduler()
    {
        if ( !m_scheduler ) {
            (void)finder();
            m_scheduler = std::make_unique<BatchScheduler>( m_source, m_finder, m_batch, m_device );
            if ( !m_finder->complete() ) {
                m_finder->startThreads();
            }
        }
        return *m_scheduler;
    }

    void
    handOffsetsToFinder( const OffsetMap& offsets )
    {
        if ( offsets.empty() ) {
            fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, "a list of block offsets is required" );
        }
        std::vector<size_t> dataBlocks;
        for ( auto entry = offsets.begin(), behind = std::next( entry ); behind != offsets.end(); ++entry, ++behind ) {
            if ( entry->second != behind->second ) {
                dataBlocks.push_back( entry->first );
            }
        }
        (void)finder().adopt( std::move( dataBlocks ), BlockFinder::Authority::CALLER );
    }

private:
    std::shared_ptr<Source> m_source;
    const size_t m_batch;
    const int m_device;
    size_t m_position{ 0 };
    bool m_atEnd{ false };

    bool m_checkStreamCrc;
    uint32_t m_streamCrc{ 0 };
    uint64_t m_streamsVerified{ 0 };

    std::shared_ptr<BlockFinder> m_finder;
    BlockIndex m_index;
    std::unique_ptr<BatchScheduler> m_scheduler;

    std::optional<LineIndex> m_lines;     /* the one line index the reader keeps, with its delimiter */
    std::optional<HeldLines> m_held;      /* between read_line_ranges and take_line_ranges */
    std::optional<std::vector<uint64_t> > m_matches;   /* between search (with a limit) and take_matches */
    struct HeldSetMatches
    {
        std::vector<uint64_t> positions;
        std::vector<uint32_t> ids;
    };
    std::optional<HeldSetMatches> m_setMatches;        /* between search_set (with a limit) and take_set_matches */
    std::optional<HeldGrep> m_grep;       /* between grep and take_line_ranges, beside m_held */
    HeldBytes m_heldBytes;                /* of m_held's pieces, per context; written by the line jobs */
    std::optional<HeldColumns> m_hashes;  /* between line_hashes and the next line_hashes / distinct_lines */
    std::optional<HeldColumns> m_fields;  /* between field_spans and the next field_spans */
    std::optional<HeldFieldColumns> m_fieldColumns;           /* between field_columns and the next field_columns */
    std::optional<HeldColumns> m_fieldHashes;                 /* between field_hashes and the next call of its family */
    std::optional<std::vector<FieldGroup> > m_fieldGroups;    /* between field_groups and the next call of its family */
    std::optional<HeldColumns> m_fieldNumbers;                /* between field_numbers and the next call of its family */
    std::optional<std::vector<FieldSumGroup> > m_fieldSums;   /* between field_sums and the next call of its family */
    std::optional<HeldFieldMatches> m_fieldMatches;           /* between field_matches / field_in_range / field_matches_regex and the next of them */
    std::optional<std::vector<uint64_t> > m_distinct;  /* between distinct_lines (with numbers) and the next of the two */
};
}  // namespace mi355x

/* ================================================================================================ C ABI */
struct mi355x_bz2_reader
{
    std::unique_ptr<mi355x::StreamReader> reader;
    std::string lastError;
};

namespace
{
template<typename Functor>
int
guarded( mi355x_bz2_reader* r, const Functor& functor )
{
    if ( r == nullptr || !r->reader ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    try {
        functor( *r->reader );
        return MI355X_BZ2_OK;
    } catch ( const mi355x::Bz2Exception& e ) {
        r->lastError = e.what();
        return e.status;
    } catch ( const std::invalid_argument& e ) {
        r->lastError = e.what();
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    } catch ( const std::exception& e ) {
        r->lastError = e.what();
        return MI355X_BZ2_ERR_LOGIC;
    }
}

template<typename MakeSource>
int
openReader( const MakeSource& makeSource, uint32_t parallelization, int32_t device, mi355x_bz2_reader** out )
{
    if ( out == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    try {
        auto source = makeSource();
        auto* r = new mi355x_bz2_reader();
        r->reader = std::make_unique<mi355x::StreamReader>( std::move( source ), parallelization, device );
        *out = r;
        return MI355X_BZ2_OK;
    } catch ( const mi355x::Bz2Exception& e ) {
        std::fprintf( stderr, "mi355x_bz2_reader_open: %s\n", e.what() );
        return e.status;
    } catch ( const std::exception& e ) {
        std::fprintf( stderr, "mi355x_bz2_reader_open: %s\n", e.what() );
        return MI355X_BZ2_ERR_LOGIC;
    }
}

int
copyOffsets( const std::map<size_t, size_t>& offsets, uint64_t* bits, uint64_t* bytes, uint64_t capacity, uint64_t* n )
{
    if ( n != nullptr ) *n = offsets.size();
    if ( capacity == 0 ) return MI355X_BZ2_OK;
    if ( bits == nullptr || bytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    uint64_t i = 0;
    for ( const auto& [b, d] : offsets ) {
        if ( i >= capacity ) break;
        bits[i] = b;
        bytes[i] = d;
        ++i;
    }
    return MI355X_BZ2_OK;
}

/** The values of a C ABI call as a table, checked before anything touches the GPU; throws std::invalid_argument. */
bz2gpu::ValueTable
takeValues( const char* what, const uint8_t* values, const uint32_t* valueSizes, uint32_t nValues, uint64_t seed )
{
    try {
        if ( nValues > 0 && valueSizes == nullptr ) throw std::invalid_argument( "no sizes for the values" );
        const auto why = bz2gpu::valueSetError( valueSizes, nValues );
        if ( !why.empty() ) throw std::invalid_argument( why );
        if ( values == nullptr && std::any_of( valueSizes, valueSizes + nValues, [] ( uint32_t size ) { return size > 0; } ) ) {
            throw std::invalid_argument( "no bytes for the values" );
        }
        return bz2gpu::valueTableOf( values, valueSizes, nValues, seed );
    } catch ( const std::invalid_argument& refused ) {
        throw std::invalid_argument( std::string( what ) + ": " + refused.what() );
    }
}
}  // namespace

extern "C" {

int
mi355x_bz2_reader_open_path( const char* path, uint32_t parallelization, int32_t device, mi355x_bz2_reader** r )
{
    if ( path == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return openReader( [path] () { return mi355x::Source::fromPath( path ); }, parallelization, device, r );
}

int
mi355x_bz2_reader_open_fd( int fd, uint32_t parallelization, int32_t device, mi355x_bz2_reader** r )
{
    /* dup so that the caller's descriptor stays usable (StandardFileReader(int), filereader/Standard.hpp:50-62) */
    return openReader( [fd] () {
        const int copy = dup( fd );
        if ( copy < 0 ) mi355x::fail( MI355X_BZ2_ERR_IO, std::string( "dup: " ) + strerror( errno ) );
        return mi355x::Source::fromFd( copy, true );
    }, parallelization, device, r );
}

int
mi355x_bz2_reader_open_memory( const uint8_t* bytes, uint64_t size, uint32_t parallelization, int32_t device,
                               mi355x_bz2_reader** r )
{
    if ( bytes == nullptr && size > 0 ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return openReader( [bytes, size] () { return mi355x::Source::fromMemory( bytes, size ); }, parallelization, device, r );
}

void
mi355x_bz2_reader_close( mi355x_bz2_reader* r )
{
    if ( r == nullptr ) return;
    if ( r->reader ) {
        try { r->reader->close(); } catch ( ... ) {}
    }
    delete r;
}

const char*
mi355x_bz2_reader_last_error( const mi355x_bz2_reader* r )
{
    return r != nullptr ? r->lastError.c_str() : "null reader";
}

int
mi355x_bz2_reader_read( mi355x_bz2_reader* r, int fd, void* buffer, uint64_t nBytes, uint64_t* nRead )
{
    if ( nRead != nullptr ) *nRead = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto n = reader.read( fd, static_cast<char*>( buffer ), (size_t)nBytes );
        if ( nRead != nullptr ) *nRead = n;
    } );
}

int
mi355x_bz2_reader_seek( mi355x_bz2_reader* r, int64_t offset, int whence, uint64_t* newPosition )
{
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto p = reader.seek( offset, whence );
        if ( newPosition != nullptr ) *newPosition = p;
    } );
}

uint64_t
mi355x_bz2_reader_tell( const mi355x_bz2_reader* r )
{
    uint64_t result = 0;
    guarded( const_cast<mi355x_bz2_reader*>( r ), [&] ( mi355x::StreamReader& reader ) { result = reader.tell(); } );
    return result;
}

int
mi355x_bz2_reader_eof( const mi355x_bz2_reader* r )
{
    return ( r != nullptr && r->reader && r->reader->eof() ) ? 1 : 0;
}

int
mi355x_bz2_reader_closed( const mi355x_bz2_reader* r )
{
    return ( r == nullptr || !r->reader || r->reader->closed() ) ? 1 : 0;
}

int
mi355x_bz2_reader_size( const mi355x_bz2_reader* r, uint64_t* size )
{
    if ( r == nullptr || !r->reader ) return 0;
    const auto s = r->reader->size();
    if ( !s ) return 0;
    if ( size != nullptr ) *size = *s;
    return 1;
}

uint64_t
mi355x_bz2_reader_tell_compressed( const mi355x_bz2_reader* r )
{
    uint64_t result = 0;
    guarded( const_cast<mi355x_bz2_reader*>( r ),
             [&] ( mi355x::StreamReader& reader ) { result = reader.tellCompressed(); } );
    return result;
}

int
mi355x_bz2_reader_block_offsets_complete( const mi355x_bz2_reader* r )
{
    return ( r != nullptr && r->reader && r->reader->indexComplete() ) ? 1 : 0;
}

int
mi355x_bz2_reader_block_offsets( mi355x_bz2_reader* r, uint64_t* bits, uint64_t* bytes, uint64_t capacity, uint64_t* n )
{
    int inner = MI355X_BZ2_OK;
    const int rc = guarded( r, [&] ( mi355x::StreamReader& reader ) {
        inner = copyOffsets( reader.blockOffsets(), bits, bytes, capacity, n );
    } );
    return rc != MI355X_BZ2_OK ? rc : inner;
}

int
mi355x_bz2_reader_available_block_offsets( const mi355x_bz2_reader* r, uint64_t* bits, uint64_t* bytes,
                                           uint64_t capacity, uint64_t* n )
{
    int inner = MI355X_BZ2_OK;
    const int rc = guarded( const_cast<mi355x_bz2_reader*>( r ), [&] ( mi355x::StreamReader& reader ) {
        inner = copyOffsets( reader.availableBlockOffsets(), bits, bytes, capacity, n );
    } );
    return rc != MI355X_BZ2_OK ? rc : inner;
}

int
mi355x_bz2_reader_set_block_offsets( mi355x_bz2_reader* r, const uint64_t* bits, const uint64_t* bytes, uint64_t n )
{
    if ( n > 0 && ( bits == nullptr || bytes == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        std::map<size_t, size_t> offsets;
        for ( uint64_t i = 0; i < n; ++i ) {
            offsets.emplace( bits[i], bytes[i] );
        }
        reader.setBlockOffsets( offsets );
    } );
}

int
mi355x_bz2_reader_read_ranges( mi355x_bz2_reader* r, const uint64_t* offsets, const uint64_t* sizes, uint32_t n, void* dst,
                               int dstIsDevice, uint64_t* nRead )
{
    if ( n > 0 && ( offsets == nullptr || sizes == nullptr || nRead == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.readRanges( offsets, sizes, n, dst, dstIsDevice != 0, nRead );
    } );
}

int
mi355x_bz2_reader_line_offsets( mi355x_bz2_reader* r, uint8_t nl, uint64_t* bytes, uint64_t* lines, uint64_t capacity,
                                uint64_t* n )
{
    if ( capacity > 0 && ( bytes == nullptr || lines == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto pairs = reader.lineOffsets( nl );
        if ( n != nullptr ) *n = pairs.size();
        for ( uint64_t i = 0; i < pairs.size() && i < capacity; ++i ) {
            bytes[i] = pairs[i].first;
            lines[i] = pairs[i].second;
        }
    } );
}

int
mi355x_bz2_reader_set_line_offsets( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* bytes, const uint64_t* lines, uint64_t n )
{
    if ( n > 0 && ( bytes == nullptr || lines == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.setLineOffsets( nl, bytes, lines, (size_t)n ); } );
}

int
mi355x_bz2_reader_line_starts( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* lines, uint32_t n, uint64_t* byteOffsets )
{
    if ( n > 0 && ( lines == nullptr || byteOffsets == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.lineStarts( nl, lines, n, byteOffsets ); } );
}

int
mi355x_bz2_reader_read_line_ranges( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* first, const uint64_t* count,
                                    uint32_t n, int keepOnDevice, uint64_t* byteSizes, uint64_t* total )
{
    if ( total != nullptr ) *total = 0;
    if ( n > 0 && ( first == nullptr || count == nullptr || byteSizes == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.readLineRanges( nl, first, count, n, keepOnDevice != 0, byteSizes, total );
    } );
}

int
mi355x_bz2_reader_take_line_ranges( mi355x_bz2_reader* r, void* dst, int dstIsDevice )
{
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeLineRanges( dst, dstIsDevice != 0 ); } );
}

/** A flag bit that no search knows fails the call before anything is launched or held. */
static void
checkSearchFlags( const char* what, uint32_t flags )
{
    if ( ( flags & ~bz2gpu::SEARCH_KNOWN_FLAGS ) == 0 ) return;
    char bits[16];
    std::snprintf( bits, sizeof( bits ), "0x%X", flags & ~bz2gpu::SEARCH_KNOWN_FLAGS );
    mi355x::fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": unknown flag bits " + bits );
}

int
mi355x_bz2_reader_search_ex( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t patternSize, uint32_t flags, uint64_t start,
                             uint64_t end, uint64_t limit, uint64_t* nMatches )
{
    if ( pattern == nullptr || nMatches == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        checkSearchFlags( "search", flags );
        reader.search( pattern, patternSize, flags, start, end, limit, nMatches );
    } );
}

int
mi355x_bz2_reader_search( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t patternSize, uint64_t start, uint64_t end,
                          uint64_t limit, uint64_t* nMatches )
{
    return mi355x_bz2_reader_search_ex( r, pattern, patternSize, 0, start, end, limit, nMatches );
}

int
mi355x_bz2_reader_take_matches( mi355x_bz2_reader* r, uint64_t* positions, uint64_t capacity )
{
    if ( capacity > 0 && positions == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeMatches( positions, capacity ); } );
}

int
mi355x_bz2_reader_line_numbers( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* offsets, uint64_t n, uint64_t* lines )
{
    if ( n > 0 && ( offsets == nullptr || lines == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.lineNumbers( nl, offsets, (size_t)n, lines ); } );
}

int
mi355x_bz2_reader_grep_ex( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t patternSize, uint32_t flags, uint8_t nl,
                           uint64_t start, uint64_t end, uint64_t maxLines, int keepOnDevice, uint64_t* nLines,
                           uint64_t* totalBytes )
{
    if ( pattern == nullptr || nLines == nullptr || totalBytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    *totalBytes = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        checkSearchFlags( "grep", flags );
        reader.grep( pattern, patternSize, flags, nl, start, end, maxLines, keepOnDevice != 0, nLines, totalBytes );
    } );
}

int
mi355x_bz2_reader_grep( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t patternSize, uint8_t nl, uint64_t start,
                        uint64_t end, uint64_t maxLines, int keepOnDevice, uint64_t* nLines, uint64_t* totalBytes )
{
    return mi355x_bz2_reader_grep_ex( r, pattern, patternSize, 0, nl, start, end, maxLines, keepOnDevice, nLines, totalBytes );
}

int
mi355x_bz2_reader_take_grep( mi355x_bz2_reader* r, uint64_t* lineNumbers, uint64_t* byteSizes, uint64_t capacity )
{
    if ( capacity > 0 && ( lineNumbers == nullptr || byteSizes == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeGrep( lineNumbers, byteSizes, capacity ); } );
}

/** The set of a reader call, its patterns folded once if the flags ask for it; a set that breaks a limit fails the call
 * with the sentence that names it, and so does an unknown flag bit. */
static bz2gpu::PatternSet
setOf( const char* what, const uint8_t* patterns, const uint32_t* sizes, uint32_t n, uint32_t flags )
{
    checkSearchFlags( what, flags );
    const auto why = bz2gpu::patternSetError( sizes, n );
    if ( !why.empty() ) mi355x::fail( MI355X_BZ2_ERR_INVALID_ARGUMENT, std::string( what ) + ": " + why );
    return bz2gpu::makePatternSet( patterns, sizes, n, ( flags & bz2gpu::SEARCH_IGNORE_CASE ) != 0 );
}

int
mi355x_bz2_reader_search_set_ex( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* patternSizes,
                                 uint32_t nPatterns, uint32_t flags, uint64_t start, uint64_t end, uint64_t limit,
                                 uint64_t* nMatches, uint64_t* perPattern )
{
    if ( patterns == nullptr || patternSizes == nullptr || nMatches == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto set = setOf( "search_set", patterns, patternSizes, nPatterns, flags );
        reader.searchSet( set, start, end, limit, nMatches, perPattern );
    } );
}

int
mi355x_bz2_reader_search_set( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* patternSizes, uint32_t nPatterns,
                              uint64_t start, uint64_t end, uint64_t limit, uint64_t* nMatches, uint64_t* perPattern )
{
    return mi355x_bz2_reader_search_set_ex( r, patterns, patternSizes, nPatterns, 0, start, end, limit, nMatches, perPattern );
}

int
mi355x_bz2_reader_take_set_matches( mi355x_bz2_reader* r, uint64_t* positions, uint32_t* ids, uint64_t capacity )
{
    if ( capacity > 0 && ( positions == nullptr || ids == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeSetMatches( positions, ids, capacity ); } );
}

int
mi355x_bz2_reader_grep_regex( mi355x_bz2_reader* r, const mi355x_bz2_regex* re, uint8_t nl, uint64_t maxLines, int keepOnDevice,
                              uint64_t* nLines, uint64_t* totalBytes )
{
    if ( re == nullptr || nLines == nullptr || totalBytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.grepRegex( re->dfa, nl, maxLines, keepOnDevice != 0, nLines, totalBytes );
    } );
}

int
mi355x_bz2_reader_line_hashes( mi355x_bz2_reader* r, uint8_t nl, uint64_t seed, uint64_t first, uint64_t count, int keepOnDevice,
                               uint64_t* nLines )
{
    if ( nLines == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.lineHashes( nl, seed, first, count, keepOnDevice != 0, nLines ); } );
}

int
mi355x_bz2_reader_take_line_hashes( mi355x_bz2_reader* r, void* hashes, uint64_t capacity, int dstIsDevice )
{
    if ( capacity > 0 && hashes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeLineHashes( hashes, capacity, dstIsDevice != 0 ); } );
}

const uint64_t*
mi355x_bz2_reader_line_hashes_device( mi355x_bz2_reader* r )
{
    return r != nullptr && r->reader ? r->reader->lineHashesDevice() : nullptr;
}

int
mi355x_bz2_reader_field_spans( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count,
                               int keepOnDevice, uint64_t* nLines )
{
    if ( nLines == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.fieldSpans( nl, dl, field, first, count, keepOnDevice != 0, nLines ); } );
}

int
mi355x_bz2_reader_take_field_spans( mi355x_bz2_reader* r, void* starts, void* sizes, uint64_t capacity, int dstIsDevice )
{
    if ( capacity > 0 && ( starts == nullptr || sizes == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldSpans( starts, sizes, capacity, dstIsDevice != 0 ); } );
}

int
mi355x_bz2_reader_field_columns( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, const uint32_t* fields, uint32_t nFields, uint64_t first,
                                 uint64_t count, int keepOnDevice, uint64_t* nLines, uint64_t* totalBytes )
{
    if ( nLines == nullptr || totalBytes == nullptr || ( nFields > 0 && fields == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    std::fill_n( totalBytes, std::min<uint32_t>( nFields, bz2gpu::FIELD_COLUMNS_MAX ), uint64_t( 0 ) );
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldColumns( nl, dl, fields, nFields, first, count, keepOnDevice != 0, nLines, totalBytes );
    } );
}

int
mi355x_bz2_reader_field_spans_quoted( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count,
                                      int keepOnDevice, uint64_t* nLines, uint8_t quote )
{
    if ( nLines == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldSpans( nl, dl, field, first, count, keepOnDevice != 0, nLines, quote );
    } );
}

int
mi355x_bz2_reader_field_columns_quoted( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, const uint32_t* fields, uint32_t nFields,
                                        uint64_t first, uint64_t count, int keepOnDevice, uint64_t* nLines, uint64_t* totalBytes,
                                        uint8_t quote )
{
    if ( nLines == nullptr || totalBytes == nullptr || ( nFields > 0 && fields == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    std::fill_n( totalBytes, std::min<uint32_t>( nFields, bz2gpu::FIELD_COLUMNS_MAX ), uint64_t( 0 ) );
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldColumns( nl, dl, fields, nFields, first, count, keepOnDevice != 0, nLines, totalBytes, quote );
    } );
}

int
mi355x_bz2_reader_take_field_column( mi355x_bz2_reader* r, uint32_t column, void* data, void* offsets, void* sizes, int dstIsDevice )
{
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldColumn( column, data, offsets, sizes, dstIsDevice != 0 ); } );
}

int
mi355x_bz2_reader_field_hashes( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first,
                                uint64_t count, int keepOnDevice, uint64_t* nLines )
{
    if ( nLines == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldHashes( nl, dl, field, seed, first, count, keepOnDevice != 0, nLines );
    } );
}

int
mi355x_bz2_reader_take_field_hashes( mi355x_bz2_reader* r, void* keys, uint64_t capacity, int dstIsDevice )
{
    if ( capacity > 0 && keys == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldHashes( keys, capacity, dstIsDevice != 0 ); } );
}

int
mi355x_bz2_reader_field_groups( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first,
                                uint64_t count, uint64_t* nGroups, uint64_t* nMissing )
{
    if ( nGroups == nullptr || nMissing == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nGroups = 0;
    *nMissing = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.fieldGroups( nl, dl, field, seed, first, count, nGroups, nMissing ); } );
}

int
mi355x_bz2_reader_take_field_groups( mi355x_bz2_reader* r, uint64_t* lines, uint64_t* counts, uint64_t* starts, int64_t* sizes,
                                     uint64_t capacity )
{
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldGroups( lines, counts, starts, sizes, capacity ); } );
}

int
mi355x_bz2_reader_field_numbers( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count,
                                 int keepOnDevice, uint64_t* nLines )
{
    if ( nLines == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nLines = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldNumbers( nl, dl, field, first, count, keepOnDevice != 0, nLines );
    } );
}

int
mi355x_bz2_reader_take_field_numbers( mi355x_bz2_reader* r, void* numbers, uint64_t capacity, int dstIsDevice )
{
    if ( capacity > 0 && numbers == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldNumbers( numbers, capacity, dstIsDevice != 0 ); } );
}

int
mi355x_bz2_reader_field_sums( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t keyField, uint32_t valueField, uint64_t seed,
                              uint64_t first, uint64_t count, uint64_t* nGroups, uint64_t* nMissing )
{
    if ( nGroups == nullptr || nMissing == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nGroups = 0;
    *nMissing = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.fieldSums( nl, dl, keyField, valueField, seed, first, count, nGroups, nMissing );
    } );
}

int
mi355x_bz2_reader_take_field_sums( mi355x_bz2_reader* r, uint64_t* lines, uint64_t* counts, uint64_t* starts, int64_t* sizes,
                                   uint64_t* numbers, uint64_t* sumsLo, int64_t* sumsHi, int64_t* mins, int64_t* maxs,
                                   uint64_t capacity )
{
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.takeFieldSums( lines, counts, starts, sizes, numbers, sumsLo, sumsHi, mins, maxs, capacity );
    } );
}

int
mi355x_bz2_reader_field_matches( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const uint8_t* values,
                                 const uint32_t* valueSizes, uint32_t nValues, uint64_t seed, int invert, uint64_t first, uint64_t count,
                                 uint64_t limit, int keepOnDevice, uint64_t* nSelected, uint64_t* nMatching )
{
    if ( nSelected == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto table = takeValues( "field_matches", values, valueSizes, nValues, seed );
        uint64_t matching = 0;
        reader.fieldMatches( nl, dl, field, table, seed, invert != 0, first, count, limit, keepOnDevice != 0, nSelected, &matching );
        if ( nMatching != nullptr ) *nMatching = matching;
    } );
}

int
mi355x_bz2_reader_field_in_range( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, int hasLo, int64_t lo, int hasHi,
                                  int64_t hi, int invert, uint64_t first, uint64_t count, uint64_t limit, int keepOnDevice,
                                  uint64_t* nSelected, uint64_t* nMatching )
{
    if ( nSelected == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        uint64_t matching = 0;
        reader.fieldInRange( nl, dl, field, bz2gpu::clipNumberRange( hasLo != 0, lo, hasHi != 0, hi ), invert != 0, first, count, limit,
                             keepOnDevice != 0, nSelected, &matching );
        if ( nMatching != nullptr ) *nMatching = matching;
    } );
}

int
mi355x_bz2_reader_take_field_matches( mi355x_bz2_reader* r, void* dst, uint64_t capacity, int dstIsDevice )
{
    if ( capacity > 0 && dst == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeFieldMatches( dst, capacity, dstIsDevice != 0 ); } );
}

int
mi355x_bz2_reader_select_lines( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const uint8_t* values,
                                const uint32_t* valueSizes, uint32_t nValues, uint64_t seed, int hasLo, int64_t lo, int hasHi, int64_t hi,
                                int invert, uint64_t first, uint64_t count, uint64_t maxLines, int keepOnDevice, uint64_t* nLines,
                                uint64_t* totalBytes )
{
    if ( nLines == nullptr || totalBytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        if ( nValues > 0 && ( hasLo != 0 || hasHi != 0 ) ) throw std::invalid_argument( "select_lines: values or a range, not both" );
        if ( nValues > 0 ) {
            const auto table = takeValues( "select_lines", values, valueSizes, nValues, seed );
            reader.selectLines( [&] ( uint64_t limit, uint64_t* nSelected, uint64_t* nMatching ) {
                reader.fieldMatches( nl, dl, field, table, seed, invert != 0, first, count, limit, false, nSelected, nMatching, "select_lines" );
            }, nl, maxLines, keepOnDevice != 0, nLines, totalBytes );
        } else {
            const auto range = bz2gpu::clipNumberRange( hasLo != 0, lo, hasHi != 0, hi );
            reader.selectLines( [&] ( uint64_t limit, uint64_t* nSelected, uint64_t* nMatching ) {
                reader.fieldInRange( nl, dl, field, range, invert != 0, first, count, limit, false, nSelected, nMatching, "select_lines" );
            }, nl, maxLines, keepOnDevice != 0, nLines, totalBytes );
        }
    } );
}

int
mi355x_bz2_reader_field_matches_regex( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const mi355x_bz2_regex* re,
                                       int invert, uint64_t first, uint64_t count, uint64_t limit, int keepOnDevice,
                                       uint64_t* nSelected, uint64_t* nMatching )
{
    if ( re == nullptr || nSelected == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        uint64_t matching = 0;
        reader.fieldMatchesRegex( nl, dl, field, re->dfa, invert != 0, first, count, limit, keepOnDevice != 0, nSelected, &matching );
        if ( nMatching != nullptr ) *nMatching = matching;
    } );
}

int
mi355x_bz2_reader_select_lines_regex( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const mi355x_bz2_regex* re,
                                      int invert, uint64_t first, uint64_t count, uint64_t maxLines, int keepOnDevice,
                                      uint64_t* nLines, uint64_t* totalBytes )
{
    if ( re == nullptr || nLines == nullptr || totalBytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        reader.selectLines( [&] ( uint64_t limit, uint64_t* nSelected, uint64_t* nMatching ) {
            reader.fieldMatchesRegex( nl, dl, field, re->dfa, invert != 0, first, count, limit, false, nSelected, nMatching,
                                      "select_lines_regex" );
        }, nl, maxLines, keepOnDevice != 0, nLines, totalBytes );
    } );
}

int
mi355x_bz2_reader_distinct_lines( mi355x_bz2_reader* r, uint8_t nl, uint64_t seed, int wantNumbers, uint64_t* nDistinct )
{
    if ( nDistinct == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *nDistinct = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.distinctLines( nl, seed, wantNumbers != 0, nDistinct ); } );
}

int
mi355x_bz2_reader_take_distinct_lines( mi355x_bz2_reader* r, uint64_t* lineNumbers, uint64_t capacity )
{
    if ( capacity > 0 && lineNumbers == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) { reader.takeDistinctLines( lineNumbers, capacity ); } );
}

int
mi355x_bz2_reader_grep_set_ex( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* patternSizes, uint32_t nPatterns,
                               uint32_t flags, uint8_t nl, uint64_t start, uint64_t end, uint64_t maxLines, int keepOnDevice,
                               uint64_t* nLines, uint64_t* totalBytes )
{
    if ( patterns == nullptr || patternSizes == nullptr || nLines == nullptr || totalBytes == nullptr ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    *nLines = 0;
    *totalBytes = 0;
    return guarded( r, [&] ( mi355x::StreamReader& reader ) {
        const auto set = setOf( "grep_set", patterns, patternSizes, nPatterns, flags );
        reader.grepSet( set, nl, start, end, maxLines, keepOnDevice != 0, nLines, totalBytes );
    } );
}

int
mi355x_bz2_reader_grep_set( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* patternSizes, uint32_t nPatterns,
                            uint8_t nl, uint64_t start, uint64_t end, uint64_t maxLines, int keepOnDevice, uint64_t* nLines,
                            uint64_t* totalBytes )
{
    return mi355x_bz2_reader_grep_set_ex( r, patterns, patternSizes, nPatterns, 0, nl, start, end, maxLines, keepOnDevice,
                                          nLines, totalBytes );
}

int
mi355x_bz2_reader_join_threads( mi355x_bz2_reader* r )
{
    return guarded( r, [] ( mi355x::StreamReader& reader ) { reader.joinThreads(); } );
}

int
mi355x_bz2_reader_set_verify_stream_crc( mi355x_bz2_reader* r, int enable )
{
    return guarded( r, [enable] ( mi355x::StreamReader& reader ) { reader.setVerifyStreamCrc( enable != 0 ); } );
}

uint64_t
mi355x_bz2_reader_streams_verified( const mi355x_bz2_reader* r )
{
    return ( r != nullptr && r->reader ) ? r->reader->streamsVerified() : 0;
}

int
mi355x_bz2_reader_statistics( const mi355x_bz2_reader* r, mi355x_bz2_reader_stats* stats )
{
    if ( stats == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return guarded( const_cast<mi355x_bz2_reader*>( r ),
                    [&] ( mi355x::StreamReader& reader ) { *stats = reader.statistics(); } );
}

}  // extern "C"
