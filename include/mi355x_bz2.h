/*
 * mi355x_bz2.h -- C ABI of the MI355X-native parallel bzip2 block decoder.
 *
 * This is the drop-in boundary for ONE path of WeGoToMars/indexed_bzip2: decoding independent bzip2 blocks behind
 * ParallelBZ2Reader / ibzip2.open().  Everything is `extern "C"`, plain pointers and sizes.  Each entry point cites
 * the reference interface it replaces (paths relative to the reference repository root).
 *
 * Layers exported here:
 *   1. Block codec on the GPU (the operator seam):      mi355x_bz2_create / _set_input_* / _decode_batch / ...
 *        replaces  BZ2BlockFetcher::decodeBlock          src/indexed_bzip2/BZ2BlockFetcher.hpp:85-138
 *                  (virtual BlockFetcher::decodeBlock    src/core/BlockFetcher.hpp:580-582)
 *        and everything it calls: bzip2::Block           src/indexed_bzip2/bzip2.hpp:145-461, 479-910
 *   2. Host magic-bit scan:                              mi355x_bz2_find_magic
 *        replaces  BitStringFinder<48>::find             src/core/BitStringFinder.hpp:158-285
 *                  ParallelBitStringFinder<48>::find     src/core/ParallelBitStringFinder.hpp:159-265
 *   3. Reader (scheduler + block map + user API):        mi355x_bz2_reader_*
 *        replaces  indexed_bzip2::ParallelBZ2Reader      src/indexed_bzip2/ParallelBZ2Reader.hpp:39-498
 *                  (BZ2ReaderInterface                   src/indexed_bzip2/BZ2ReaderInterface.hpp:15-103)
 *        as bound by the Cython module                   python/indexed_bzip2/indexed_bzip2.pyx:26-67
 *   4. Chunk decoding for rapidgzip:                     mi355x_bz2_decode_chunk
 *        replaces  Bzip2Chunk::decodeChunk               src/rapidgzip/chunkdecoding/Bzip2Chunk.hpp:34-268
 *
 * No exceptions cross this ABI: every reference throw site on the path has a status code below; the host-side
 * scheduler turns a non-OK status back into the reference's behaviour (prefetch failures are silent, on-demand
 * failures surface from read(); src/core/BlockFetcher.hpp:305, 424-432).
 *
 * Threads.  A mi355x_bz2_ctx and a mi355x_bz2_reader are each used by ONE thread at a time: their calls are not
 * serialised against one another, and a result held between a step-1 call and its take belongs to the calls of that
 * one thread.  Different contexts and readers on different threads are independent of one another, also on the same
 * device, also while one of them is created or destroyed under another's batch in flight: what they share -- per
 * device the chain that orders their walks, the count of live contexts from which every batch takes its lane layout
 * and its crowd mode, and the once-per-device kernel attributes -- is guarded inside the library; the distinct-lines and
 * group-by calls sort on the null stream, which the threads of a process share, each call in device memory of its own
 * that it allocates and frees; and every entry point sets the calling thread's current HIP device itself.  The number
 * of live contexts changes a batch's launch plan and never its result.  mi355x_bz2_find_magic, the status and name
 * functions and mi355x_bz2_warmup may be called from any thread.  The MI355X_BZ2_* environment switches are read with
 * getenv while the library runs (per batch, per reader launch): the environment must not be changed while another
 * thread is inside the library.  tests/test_gpu_threads.py pins all of this.
 */
#ifndef MI355X_BZ2_H
#define MI355X_BZ2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_BZ2_ABI_VERSION 2

/* ------------------------------------------------------------------------------------------------ status codes */
typedef enum mi355x_bz2_status {
    MI355X_BZ2_OK = 0,
    MI355X_BZ2_ERR_EOF = 1,               /* BitReader::EndOfFileReached            src/core/BitReader.hpp:82-84 */
    MI355X_BZ2_ERR_BAD_MAGIC = 2,         /* "invalid compressed magic"             bzip2.hpp:502-507 */
    MI355X_BZ2_ERR_RANDOMIZED = 3,        /* "isRandomized bit is not supported"    bzip2.hpp:509-512 */
    MI355X_BZ2_ERR_ORIGPTR_RANGE = 4,     /* "origPtr ... larger than buffer size"  bzip2.hpp:514-519 */
    MI355X_BZ2_ERR_GROUP_COUNT = 5,       /* "Invalid Huffman coding group count"   bzip2.hpp:579-583 */
    MI355X_BZ2_ERR_SELECTOR_COUNT = 6,    /* "number of selectors ... invalid"      bzip2.hpp:593-597 */
    MI355X_BZ2_ERR_SELECTOR_UNARY = 7,    /* "Could not find zero termination"      bzip2.hpp:625-629 */
    MI355X_BZ2_ERR_CODE_LENGTH = 8,       /* "start_huffman_length ..."             bzip2.hpp:657-662 */
    MI355X_BZ2_ERR_HUFFMAN_LENGTHS = 9,   /* Error::INVALID_CODE_LENGTHS            bzip2.hpp:680-683 */
    MI355X_BZ2_ERR_SELECTOR_OVERRUN = 10, /* "selector ... out of maximum range"    bzip2.hpp:714-718 */
    MI355X_BZ2_ERR_INVALID_CODE = 11,     /* std::bad_optional_access               bzip2.hpp:723 */
    MI355X_BZ2_ERR_RUN_OVERFLOW = 12,     /* "dbufCount + hh ... > dbufSize"        bzip2.hpp:751-756 */
    MI355X_BZ2_ERR_DATA_OVERFLOW = 13,    /* "dbufCount ... > dbufSize"             bzip2.hpp:776-780 */
    MI355X_BZ2_ERR_ORIGPTR_DATA = 14,     /* "origPtr error"                        bzip2.hpp:794-798 */
    MI355X_BZ2_ERR_CRC = 15,              /* "Calculated CRC ... mismatches"        bzip2.hpp:900-907 */
    MI355X_BZ2_ERR_STREAM_HEADER = 16,    /* readBzip2Header                        bzip2.hpp:114-142 */
    MI355X_BZ2_ERR_STREAM_CRC = 17,       /* "Stream CRC ... does not match"        BZ2Reader.hpp:406-416 */
    MI355X_BZ2_ERR_NO_BLOCK_IN_RANGE = 18,/* rapidgzip::NoBlockInRange              Bzip2Chunk.hpp:262-266 */

    /* errors of this implementation, no reference counterpart */
    MI355X_BZ2_ERR_OUTPUT_CAPACITY = 100,
    MI355X_BZ2_ERR_DEVICE = 101,          /* HIP runtime error (see mi355x_bz2_last_error) */
    MI355X_BZ2_ERR_NO_DEVICE = 102,       /* no gfx950 device / HIP extension unusable: the product path has NO CPU fallback */
    MI355X_BZ2_ERR_INVALID_ARGUMENT = 103,
    MI355X_BZ2_ERR_IO = 104,
    MI355X_BZ2_ERR_CLOSED = 105,
    MI355X_BZ2_ERR_LOGIC = 106
} mi355x_bz2_status;

const char* mi355x_bz2_status_string( int status );
int mi355x_bz2_abi_version( void );

/* ------------------------------------------------------------------------------------------------ 1. block codec */

typedef struct mi355x_bz2_ctx mi355x_bz2_ctx;

typedef struct mi355x_bz2_config {
    int32_t  device;              /* HIP device ordinal; -1 = current device */
    uint32_t max_batch_blocks;    /* initial scratch capacity in blocks (grows on demand); 0 = default 64 */
    uint32_t flags;               /* MI355X_BZ2_FLAG_* */
    uint32_t reserved;
} mi355x_bz2_config;

#define MI355X_BZ2_FLAG_KEEP_STAGES 1u   /* keep per-stage buffers addressable for mi355x_bz2_debug_copy_stage */

/* Mirrors indexed_bzip2::BlockData / BlockHeaderData (src/indexed_bzip2/BZ2BlockFetcher.hpp:18-34); `data` is the
 * byte range [data_offset, data_offset + decoded_size) of the batch output buffer. */
typedef struct mi355x_bz2_block_result {
    uint64_t encoded_offset_bits;   /* BlockHeaderData::encodedOffsetInBits */
    uint64_t encoded_size_bits;     /* BlockHeaderData::encodedSizeInBits */
    uint64_t decoded_size;          /* BlockData::data.size()  (D) */
    uint64_t data_offset;           /* offset of this block's bytes in the batch output buffer */
    uint32_t header_crc;            /* BlockHeaderData::expectedCRC (stream CRC for an EOS block) */
    uint32_t computed_crc;          /* BlockData::calculatedCRC */
    uint32_t bwt_length;            /* N: symbols in dbuf after readBlockData (roofline accounting) */
    uint32_t orig_ptr;
    uint32_t n_symbols;             /* Huffman symbols decoded incl. end-of-block */
    int32_t  is_eos;                /* BlockHeaderData::isEndOfStreamBlock */
    int32_t  is_eof;                /* BlockHeaderData::isEndOfFile */
    int32_t  status;                /* mi355x_bz2_status */
} mi355x_bz2_block_result;

/* Device time of every kernel launch of the last decode_batch, measured with HIP events recorded on the ctx stream
 * around each launch (the stream the kernels run on).  Kernel i is named by mi355x_bz2_kernel_name(i). */
#define MI355X_BZ2_MAX_KERNELS 16
typedef struct mi355x_bz2_timings {
    float    ms_total;                           /* first kernel start .. last kernel end (includes the one host sync) */
    float    ms_kernel_sum;                      /* sum of ms_kernel[] */
    uint32_t n_kernels;
    uint32_t reserved;
    float    ms_kernel[MI355X_BZ2_MAX_KERNELS];
} mi355x_bz2_timings;

const char* mi355x_bz2_kernel_name( uint32_t index );

/* Create / destroy a decoder context bound to one GPU and one HIP stream.
 * Fails with MI355X_BZ2_ERR_NO_DEVICE when no usable gfx950 device exists: there is no CPU fallback. */
int  mi355x_bz2_create( const mi355x_bz2_config* config, mi355x_bz2_ctx** ctx );
/* Optional: pay the one-time cost of the HIP runtime and of loading this library's kernels (0.2 s per process, otherwise
 * part of the first mi355x_bz2_create / the first launch) at a moment of the caller's choosing, e.g. on a thread while
 * the application starts.  No reference counterpart (the reference's thread pool starts lazily too, BlockFetcher.hpp:620);
 * never needed for correctness.  Do not call it in a process that forks workers afterwards. */
int  mi355x_bz2_warmup( int32_t device );
void mi355x_bz2_destroy( mi355x_bz2_ctx* ctx );
const char* mi355x_bz2_last_error( const mi355x_bz2_ctx* ctx );

/* Make the compressed file (or any byte range of it; bit offsets below are relative to `bytes[0]`) resident in HBM.
 * All forms COPY into ctx-owned memory, in file byte order: the kernels read the stream with 16-byte loads and no bounds
 * checks, so the copy is zero padded by >= 256 bytes (they swap each 32-bit word as they load it; there is no swapped
 * copy and no swap pass).  _host copies H2D (pageable or page-locked host memory) and waits; _device copies D2D from a
 * device pointer that is only read during the call (size need not be padded).  The caller's buffer may be freed
 * afterwards; the copy costs `size` bytes of HBM.
 * _host_async only QUEUES the H2D copy (in 64-MiB pieces, on a stream of the context's own) and returns: the next
 * decode_batch[_begin] on this context is ordered behind it, so the transfer overlaps with whatever is running.  It may
 * be called while a batch is in flight on this context -- these are then the bytes of the NEXT batch, copied into a second
 * buffer beside the kernels of the current one (what bench.py does).  `bytes` should be page-locked (hipHostMalloc /
 * hipHostRegister) and must stay valid until that batch's decode_batch_end has returned.
 * Replaces the BitReader/SharedFileReader clone + pread of BZ2BlockFetcher.hpp:89-90. */
int mi355x_bz2_set_input_host( mi355x_bz2_ctx* ctx, const uint8_t* bytes, uint64_t size );
int mi355x_bz2_set_input_host_async( mi355x_bz2_ctx* ctx, const uint8_t* bytes, uint64_t size );
/* _host_streamed returns at once and copies in the background, in 32-MiB pieces on a thread and a stream of its own
 * (pageable memory is fine: a memory-mapped file): every decode_batch[_begin] waits only for the pieces in which its
 * blocks lie, so the first blocks of a large file decode while the rest is still on its way
 * (mi355x_bz2_find_magic_device needs all of it and waits for all of it).  `bytes` must stay valid until
 * mi355x_bz2_input_resident returns 1, the next set_input_* or the destruction of the context.  Contexts that share the
 * input (mi355x_bz2_share_input) share the copy in progress. */
int mi355x_bz2_set_input_host_streamed( mi355x_bz2_ctx* ctx, const uint8_t* bytes, uint64_t size );
int mi355x_bz2_input_resident( const mi355x_bz2_ctx* ctx );
int mi355x_bz2_set_input_device( mi355x_bz2_ctx* ctx, const void* device_bytes, uint64_t size );
/* Several contexts over ONE resident copy of the input (the reader keeps two contexts to overlap consecutive batches):
 * `ctx` decodes from the bytes `from` made resident.  Nothing is copied; `from` must outlive `ctx`'s use of them and
 * keep its input unchanged.  Both contexts must be on the same device. */
int mi355x_bz2_share_input( mi355x_bz2_ctx* ctx, mi355x_bz2_ctx* from );

/* A batch holds at most this many blocks (grid dimensions and 16-bit segment ids are sized for it; 65 535 level-9
 * blocks are 59 GB of decoded data and 850 GB of scratch): larger requests fail with MI355X_BZ2_ERR_INVALID_ARGUMENT. */
#define MI355X_BZ2_MAX_BATCH_BLOCKS 65535u

/* Decode n_blocks independent blocks whose magic starts at block_bit_offsets[i] (from the finder or the index).
 * = n calls of BZ2BlockFetcher::decodeBlock (BZ2BlockFetcher.hpp:85-138).  An offset pointing at an EOS magic
 * returns is_eos=1 and no data (ibid. :101-104).  results[i].status reports per-block failures; the function's
 * own return value is non-OK only for argument/device failures.  Decoded bytes stay in HBM (ctx-owned, valid
 * until the next decode_batch/destroy); *total_decoded = sum of decoded_size. */
int mi355x_bz2_decode_batch( mi355x_bz2_ctx* ctx, const uint64_t* block_bit_offsets, uint32_t n_blocks,
                             mi355x_bz2_block_result* results, uint64_t* total_decoded );

/* The same in two halves, for callers that keep the GPU busy across batches.
 *   _begin plans the batch and queues ALL of it without waiting: the group-start scan, symbols, MTF, table build, walk,
 *          the output offsets (computed on the device, k_offsets), the run-length expansion into the output buffer, the
 *          CRC, and the copy of the block records to the host.  The output buffer is chosen here for 900 000 bytes per
 *          block; a mi355x_bz2_hold_output_until event given before _begin is waited for by the output kernels only.
 *   _end   waits for the batch and fills `results` (n entries, in the order given to _begin).  Only when the batch
 *          decoded to more than the buffer chosen in _begin (blocks beyond the usual 900 000 bytes) does it repeat the
 *          expansion and the CRC with a buffer of the right size.
 * One batch per context can be in flight; contexts used in turn (begin(A), begin(B), end(A), begin(A'), end(B), ...)
 * overlap the latency-bound first kernels of one batch with the throughput kernels of the others.  The input of the NEXT
 * batch may be queued while one is in flight (mi355x_bz2_set_input_host_async: second input buffer, stream of its own).
 * Block groups and, for small batches, the second k_mtf instance of a group run on streams of their own as far as the
 * context's share of the hardware queues allows: GPU_MAX_HW_QUEUES (as the runtime reads it, 4 by default) divided by the
 * contexts alive on the device.  A context whose share is one queue runs a batch as one group on its own stream.  Input
 * copies, output copies and the device magic scan have a stream each. */
int mi355x_bz2_decode_batch_begin( mi355x_bz2_ctx* ctx, const uint64_t* block_bit_offsets, uint32_t n_blocks );
int mi355x_bz2_decode_batch_end( mi355x_bz2_ctx* ctx, mi355x_bz2_block_result* results, uint64_t* total_decoded );

/* Device pointer of the last batch's ragged output buffer (block i at data_offset).  After mi355x_bz2_decompress_buffers
 * this function, mi355x_bz2_copy_output and mi355x_bz2_gather_output address that call's result instead (the buffers'
 * bytes back to back), until the next batch or call on the context. */
const void* mi355x_bz2_output_device( const mi355x_bz2_ctx* ctx );
/* Copy [offset, offset+size) of the last batch's output to host memory (D2H). */
int mi355x_bz2_copy_output( mi355x_bz2_ctx* ctx, uint64_t offset, uint64_t size, void* host_dst );
/* The same copy in the background, on a stream of its own: _begin (after decode_batch_end, before the next
 * decode_batch_begin; not for the result of mi355x_bz2_decompress_buffers: MI355X_BZ2_ERR_INVALID_ARGUMENT) queues it and returns, _end waits for the copy started last.  The context then writes its next
 * batch into a second output buffer, so the next decode_batch_begin may follow at once: the copy of batch k overlaps the
 * kernels of batch k + 1 (the reader's per-context loop; ParallelBZ2Reader gets the same overlap from its thread pool,
 * BlockFetcher.hpp:620-642).  `host_dst` should be page-locked and must stay valid until _end has returned.
 * mi355x_bz2_output_device keeps pointing at the batch finished last. */
int mi355x_bz2_copy_output_begin( mi355x_bz2_ctx* ctx, uint64_t offset, uint64_t size, void* host_dst );
/* For callers that read mi355x_bz2_output_device themselves, asynchronously (a collective that sends the decoded extent
 * to another GPU): `hip_event` (a hipEvent_t recorded behind that read) is waited for by the context's stream before the
 * NEXT batch writes its output -- not before its other kernels.  The event is not owned and must stay valid until the next
 * decode_batch_end has returned.  Call between decode_batch_end and the next decode_batch_begin. */
int mi355x_bz2_hold_output_until( mi355x_bz2_ctx* ctx, void* hip_event );
int mi355x_bz2_copy_output_end( mi355x_bz2_ctx* ctx );
int mi355x_bz2_last_timings( const mi355x_bz2_ctx* ctx, mi355x_bz2_timings* timings );
/* Only the duration of the last batch's kernel pipeline (HIP events before the first and after the last kernel): one
 * event query instead of the ~90 that the per-kernel breakdown of mi355x_bz2_last_timings needs. */
int mi355x_bz2_last_pipeline_ms( const mi355x_bz2_ctx* ctx, float* milliseconds );
/* The hipStream_t the context launches on (as void*), so callers can order their own work after it. */
void* mi355x_bz2_stream( const mi355x_bz2_ctx* ctx );
/* Device memory the context holds right now: the per-block scratch (sized by the largest batch so far) and its output
 * buffers (sized by the largest batch's decoded bytes; two once a background copy has been used).  Either pointer may
 * be NULL.  No counterpart in the reference (its decoders keep ~5 bytes per decoded byte on the heap, bzip2.hpp:425-441). */
int mi355x_bz2_device_memory( const mi355x_bz2_ctx* ctx, uint64_t* scratch_bytes, uint64_t* output_bytes );

/* Debug/parity hook (needs MI355X_BZ2_FLAG_KEEP_STAGES -- without it stages 0 and 2 share their memory and are refused): copy an intermediate stage of block `index` of the last
 * batch to host. stage 0 = L column (N bytes, bzip2.hpp:789 dbuf low bytes), 1 = packed LF table (4N bytes),
 * 2 = inverse-BWT output before RLE1 (N bytes). */
int mi355x_bz2_debug_copy_stage( mi355x_bz2_ctx* ctx, uint32_t index, int stage, void* host_dst, uint64_t capacity );

/* bzip2's CRC-32 (MSB-first, polynomial 0x04C11DB7, createCRC32LookupTable / updateCRC32, bzip2.hpp:59-91, with the
 * initial value and final inversion of bzip2.hpp:833, 901) of `n_pieces` consecutive pieces of a DEVICE buffer: piece i
 * is the `sizes[i]` bytes behind the pieces in front of it.  For consumers of decoded extents that sit on another GPU
 * (the gather of bench.py): the receiver recomputes every block's checksum over the bytes that ARRIVED and compares it
 * with the checksum the sender's block record carries.  `device_bytes` must be 16-byte aligned; runs on the context's
 * stream and waits for the result; no batch may be in flight on the context.  A piece may have any size that fits
 * uint64_t, 2^32 bytes and more included: the checksum is exact.  One workgroup walks a piece serially, so the time
 * of a call is that of its largest piece. */
int mi355x_bz2_crc32_device( mi355x_bz2_ctx* ctx, const void* device_bytes, const uint64_t* sizes, uint32_t n_pieces,
                             uint32_t* crcs );

/* Pieces of the last batch's output (mi355x_bz2_output_device) copied into `dst` by the k_gather kernel: piece i is
 * [src_offset, src_offset + size) of the output, written to dst + dst_offset.  `dst` is device memory on the context's
 * device (dst_is_device = 1) or host memory (dst_is_device = 0: the pieces are gathered back to back into a context-owned
 * device staging buffer, copied to the host in one D2H and put in place; bytes of `dst` that no piece covers are not
 * written).  Offsets and sizes may have any alignment.  Runs on the context's stream and returns when done; no batch may
 * be in flight.  The read_ranges path of the reader; no reference counterpart. */
typedef struct mi355x_bz2_gather_piece {
    uint64_t src_offset, dst_offset, size;
} mi355x_bz2_gather_piece;
int mi355x_bz2_gather_output( mi355x_bz2_ctx* ctx, const mi355x_bz2_gather_piece* pieces, uint32_t n_pieces,
                              void* dst, int dst_is_device );

/* One byte value in spans of the last batch's output (mi355x_bz2_output_device), on the GPU: the kernels under the
 * reader's newline index and line ranges.  The same rules as mi355x_bz2_gather_output: the spans lie inside the last
 * batch's output (else MI355X_BZ2_ERR_INVALID_ARGUMENT) at any alignment, the work runs on the context's stream, the
 * calls return when it is done, and no batch may be in flight.  Spans are cut into 64-KiB tiles, one workgroup each, so a
 * span of any length is counted in parallel and searched without walking it; a span given several times is counted
 * once.  No reference counterpart for bzip2 (rapidgzip counts newlines per chunk on the host,
 * src/rapidgzip/ParallelGzipReader.hpp:1056-1145).
 *   _count_byte  counts[i] = the number of bytes equal to `value` in [offset, offset + size) of span i  (k_count_byte).
 *   _find_byte   positions[i] = the offset in the output of the rank-th (1-based; 0 is refused) byte equal to `value`
 *                in span i, or UINT64_MAX if the span holds fewer than rank of them  (k_count_byte, then k_find_byte).
 *   _rank_byte   the inverse: ranks[i] = the number of bytes equal to `value` in [offset, position) of the output, for
 *                offset <= position <= offset + size (anything else is MI355X_BZ2_ERR_INVALID_ARGUMENT); a position at
 *                the span's end gives the span's count.  Queries come in any order.  k_count_byte, then k_rank_byte with
 *                one wave per 64-KiB tile that holds a position: a tile is read once however many positions fall into
 *                it.  The call's lists take 12 bytes per position beside the tiles, in page-locked and in device memory
 *                that the context keeps until it is destroyed, like the lists of the other byte calls (grow-only; a call
 *                whose lists need more than 64 MiB and do not fit gets new buffers of that need and an eighth, a smaller
 *                one of twice the present size, or its need if that is more): ten million positions in
 *                one call leave the context with about 135 MB of each.  ranks[] is written only once every query has
 *                passed its check. */
typedef struct mi355x_bz2_byte_span {
    uint64_t offset, size;
} mi355x_bz2_byte_span;
typedef struct mi355x_bz2_byte_query {
    uint64_t offset, size, rank;
} mi355x_bz2_byte_query;
typedef struct mi355x_bz2_rank_query {
    uint64_t offset, size, position;
} mi355x_bz2_rank_query;
int mi355x_bz2_count_byte( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t value,
                           uint64_t* counts );
int mi355x_bz2_find_byte( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_query* queries, uint32_t n, uint8_t value,
                          uint64_t* positions );
int mi355x_bz2_rank_byte( mi355x_bz2_ctx* ctx, const mi355x_bz2_rank_query* queries, uint32_t n, uint8_t value,
                          uint64_t* ranks );

/* A byte string in spans of the last batch's output, on the GPU: the kernels under the reader's search.  The same rules
 * as mi355x_bz2_count_byte.  pattern_size is 1 to 256 (else MI355X_BZ2_ERR_INVALID_ARGUMENT).  A match of span i is every
 * offset p of the output with output[p : p + pattern_size] == pattern, offset <= p and p + pattern_size <= offset + size:
 * no byte outside the span decides anything, a span shorter than the pattern has none, and matches that overlap
 * themselves all count.  The start positions of a span are cut into 16-KiB tiles, one wave each; a span given twice is
 * searched twice.
 *   _count_bytes  counts[i] = the matches of span i  (k_count_bytes).
 *   _find_bytes   the same counts, and positions[] = the matches' offsets in the output, span by span in caller order and
 *                 ascending within a span, the first `capacity` of them (k_count_bytes, k_scan_tiles, k_emit_bytes: the
 *                 order comes from prefix sums, the same call gives the same array).  counts[i] is the true count of
 *                 span i whatever the capacity.  If the positions do not fit on the device the call fails with
 *                 MI355X_BZ2_ERR_DEVICE; nothing is truncated silently.
 * The _ex forms take `flags`, a union of MI355X_BZ2_SEARCH_* bits; the plain forms are the _ex forms with flags 0.  Any
 * other bit is MI355X_BZ2_ERR_INVALID_ARGUMENT before anything is launched, and mi355x_bz2_last_error names the bits.
 *   MI355X_BZ2_SEARCH_IGNORE_CASE  two bytes are equal if they are equal after b -> b | 0x20 for 'A' <= b <= 'Z' (every
 *                 other byte, 0x80 .. 0xFF included, stays as it is: bytes.lower() of Python, `LC_ALL=C grep -i`).  The
 *                 pattern may be given in any case.  Nothing else changes: spans, overlaps, order and capacity as above
 *                 (the folding instantiations of the same kernels, which read the same bytes). */
#define MI355X_BZ2_SEARCH_IGNORE_CASE 1u
int mi355x_bz2_count_bytes( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                            uint32_t pattern_size, uint64_t* counts );
int mi355x_bz2_find_bytes( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                           uint32_t pattern_size, uint64_t* positions, uint64_t capacity, uint64_t* counts );
int mi355x_bz2_count_bytes_ex( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                               uint32_t pattern_size, uint32_t flags, uint64_t* counts );
int mi355x_bz2_find_bytes_ex( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                              uint32_t pattern_size, uint32_t flags, uint64_t* positions, uint64_t capacity,
                              uint64_t* counts );

/* A SET of byte strings in spans of the last batch's output, in one pass over the bytes: the kernels under the reader's
 * search_set.  `patterns` is the concatenation of the n_patterns patterns in set order, pattern_sizes[i] the size m_i of
 * pattern i.  1 <= n_patterns <= 1024, 1 <= m_i <= 256 and the sum of the m_i <= 16384, else
 * MI355X_BZ2_ERR_INVALID_ARGUMENT before anything is launched (mi355x_bz2_last_error names the limit that was broken).
 * Equal patterns and patterns that are prefixes of one another are allowed; each reports its own matches.  A match of span
 * s is a pair (p, i) with output[p : p + m_i] == pattern i, offset <= p and p + m_i <= offset + size -- the end rule per
 * pattern: near the end of a span a short pattern still matches where a long one no longer fits.  The matches of pattern
 * i are exactly those of mi355x_bz2_find_bytes for it.  Otherwise the rules of _count_bytes / _find_bytes: the spans lie
 * inside the last batch's output, no batch may be in flight, a span given twice is searched twice.
 *   _count_bytes_set  counts[s] = the pairs of span s; per_pattern[i] (may be NULL) = the pairs of pattern i over all
 *                     spans  (k_count_set).
 *   _find_bytes_set   the same, and positions[] / ids[] = the pairs, span by span in caller order and by ascending
 *                     (position, id) within a span, the first `capacity` of them (k_count_set, k_scan_tiles, k_emit_set:
 *                     the order comes from prefix sums, the same call gives the same arrays).  The counts are true
 *                     whatever the capacity.  If the pairs do not fit on the device the call fails with
 *                     MI355X_BZ2_ERR_DEVICE; nothing is truncated silently.
 * The _ex forms take the flags of _count_bytes_ex.  With MI355X_BZ2_SEARCH_IGNORE_CASE a pair is (p, i) with output[p :
 * p + m_i] equal to pattern i under the fold; patterns that are equal under the fold, or prefixes of one another under
 * it, each report their own pairs, and the order stays (position, id). */
int mi355x_bz2_count_bytes_set( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                                const uint32_t* pattern_sizes, uint32_t n_patterns, uint64_t* counts, uint64_t* per_pattern );
int mi355x_bz2_find_bytes_set( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                               const uint32_t* pattern_sizes, uint32_t n_patterns, uint64_t* positions, uint32_t* ids,
                               uint64_t capacity, uint64_t* counts, uint64_t* per_pattern );
int mi355x_bz2_count_bytes_set_ex( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n,
                                   const uint8_t* patterns, const uint32_t* pattern_sizes, uint32_t n_patterns,
                                   uint32_t flags, uint64_t* counts, uint64_t* per_pattern );
int mi355x_bz2_find_bytes_set_ex( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n,
                                  const uint8_t* patterns, const uint32_t* pattern_sizes, uint32_t n_patterns,
                                  uint32_t flags, uint64_t* positions, uint32_t* ids, uint64_t capacity, uint64_t* counts,
                                  uint64_t* per_pattern );

/* A regular expression, compiled to a small DFA on the host (no GPU is needed), and the lines of spans of the last batch's
 * output that match it.  D, nl and lines as under line access below; the CONTENT of a line is its bytes without the
 * closing nl, and the unterminated tail is a line only if it is non-empty.  A line matches iff Python's
 * re.search( pattern, content, re.DOTALL ) on bytes finds a match; with MI355X_BZ2_SEARCH_IGNORE_CASE in `flags`,
 * re.IGNORECASE as well (ASCII letters only, 0x80 .. 0xFF never fold).  One difference: `$` is the end of the content
 * only, where Python's also matches in front of a final "\n" of the content (which a content has only if nl is not "\n").
 * Accepted syntax, every construct with Python's meaning: literal bytes, 0x80 .. 0xFF included; a backslash in front of
 * ASCII punctuation; \n \r \t \f \v \0 \xHH; \d \D \w \W \s \S; `.` (any byte); [...] and [^...] with ranges, escapes and
 * \d \w \s inside (a `]` must be escaped); ( ) and (?: ), both only grouping; |; * + ? {m} {m,} {m,n} {,n} with counts
 * <= 255; ^ and $ anywhere.  Refused with MI355X_BZ2_ERR_INVALID_ARGUMENT and a sentence in `error` (at most
 * error_capacity bytes with the final 0; may be NULL) that names the construct and its offset in the pattern:
 * back-references, look-around, inline flags, named groups, lazy and possessive quantifiers, \b \B \A \Z and every other
 * escape, a `{` that opens no repetition, an empty pattern, a pattern over 4096 bytes, any flag bit but
 * MI355X_BZ2_SEARCH_* ("unknown flag bits", as _search_ex), and a pattern whose minimal DFA has more than
 * MI355X_BZ2_REGEX_MAX_STATES states (the sentence gives the count; the construction stops at 2048 states before
 * minimisation).
 * The DFA: transitions[n][256] and accepts_at_end[n], n = _regex_states.  State 0 is the start of a line -- no transition
 * leads to it --, state 1 is "this line has matched" and is absorbing.  `^` holds in state 0 only, `$` is accepts_at_end.
 * The table does not know nl: transitions on nl are never taken.
 *   _regex_table        copies both arrays (n * 256 and n bytes).
 *   _regex_chunk_bytes  the bytes one GPU lane walks (bz2_regex.hip.h says why 256): of interest to tests and tuning.
 *   _match_lines        over spans as for _find_bytes (inside the last batch's output, no batch in flight, a span given
 *                       twice is searched twice).  Per span i, with the span read as a stretch of D that a line may enter
 *                       and leave: head_maps[64 i + q] = the state behind the span's HEAD (its bytes in front of its first
 *                       nl, all of them if it has none) entered in state q (0 for q >= n); has_delimiter[i]; exit_states[i]
 *                       = the state behind the bytes that follow the span's last nl (0 without one); counts[i] = the lines
 *                       that START inside the span and are seen to match inside it, and positions[] = one offset of the
 *                       output inside each of them (the byte that completes the first match, or the closing nl where only
 *                       the end of the line decides), span by span in caller order and ascending within a span, the first
 *                       `capacity` of them; capacity 0 runs no emitting pass.  The span's head line is not among them:
 *                       whether it matches depends on the state the span is entered in, which the caller composes
 *                       (bz2_regex.hpp: stitchSummaries).  k_regex_chunks, k_regex_link, k_scan_tiles, k_regex_emit. */
#define MI355X_BZ2_REGEX_MAX_STATES 64
typedef struct mi355x_bz2_regex mi355x_bz2_regex;
int mi355x_bz2_regex_compile( const uint8_t* pattern, uint64_t size, uint32_t flags, mi355x_bz2_regex** re, char* error,
                              uint64_t error_capacity );
void mi355x_bz2_regex_free( mi355x_bz2_regex* re );
uint32_t mi355x_bz2_regex_states( const mi355x_bz2_regex* re );
int mi355x_bz2_regex_table( const mi355x_bz2_regex* re, uint8_t* transitions, uint8_t* accepts_at_end );
uint32_t mi355x_bz2_regex_chunk_bytes( void );
int mi355x_bz2_match_lines( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, const mi355x_bz2_regex* re,
                            uint8_t nl, uint8_t* head_maps, uint8_t* has_delimiter, uint8_t* exit_states, uint64_t* positions,
                            uint64_t capacity, uint64_t* counts );

/* One 61-bit hash per line.  p = 2^61 - 1; splitmix64( s ): z = s + 0x9E3779B97F4A7C15, z = ( z ^ z >> 30 ) *
 * 0xBF58476D1CE4E5B9, z = ( z ^ z >> 27 ) * 0x94D049BB133111EB, z ^ z >> 31, all mod 2^64; the base of a 64-bit seed is
 * x = 256 + splitmix64( seed ) mod ( p - 256 ).  The hash of a line is the hash of its CONTENT (its bytes without the
 * closing nl): h = 0, then h = ( h * x + b + 1 ) mod p for every byte b, the canonical value in [0, p).  The empty line
 * hashes to 0, and "\0" and "\0\0" differ.  Two distinct contents of at most L bytes have the same hash for at most L of
 * the p - 256 bases: equal hashes say "the same line" with that probability, not with certainty, "distinct" below means
 * "of distinct hash", and a second seed is an independent check.  Lines are numbered as grep numbers them: line k is
 * closed by the k-th nl, counted from 0; a non-empty unterminated tail is one more line, an empty one is none.
 *   _line_hash        the hash of `size` bytes of content; host only, no GPU is needed.
 *   _line_hash_chunk_bytes  the bytes one GPU lane walks: of interest to tests and tuning.
 *   _hash_lines       over spans as for _find_bytes (inside the last batch's output, no batch in flight).  With
 *                     xl = x^length mod p beside a hash, ( h1, xl1 ) followed by ( h2, xl2 ) is ( h1 * xl2 + h2,
 *                     xl1 * xl2 ).  Per span i, read as a stretch of D that a line may enter and leave: head = ( h, xl ) of
 *                     its bytes in front of its first nl (all of them if it has none); has_delimiter; tail = ( h, xl ) of
 *                     the bytes behind its last nl (( 0, 1 ) without one); tail_non_empty = the span is not empty and its
 *                     last byte is not nl; count = the lines the span closes.  hashes_device[] (DEVICE memory, uint64,
 *                     room for `capacity`) receives the hashes of the closed lines, span by span in caller order and in
 *                     line order within a span, the first `capacity` of them; nothing is written at or beyond `capacity`,
 *                     and capacity 0 runs no emitting pass.  The first closed line of a span is hashed as if the span
 *                     were entered with hash 0: the caller that knows the carry ( h, xl ) in front of the span replaces
 *                     it by carry.h * head_xl + head_hash (bz2_linehash.hpp: stitchSummaries).  The call returns when
 *                     the hashes are written.  k_linehash_chunks, k_linehash_link, k_scan_tiles, k_linehash_emit. */
typedef struct mi355x_bz2_line_hash_summary
{
    uint64_t head_hash, head_xl, tail_hash, tail_xl, count;
    uint32_t has_delimiter, tail_non_empty;
} mi355x_bz2_line_hash_summary;
uint64_t mi355x_bz2_line_hash( const uint8_t* bytes, uint64_t size, uint64_t seed );
uint32_t mi355x_bz2_line_hash_chunk_bytes( void );
int mi355x_bz2_hash_lines( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint64_t seed,
                           mi355x_bz2_line_hash_summary* summaries, uint64_t* hashes_device, uint64_t capacity );

/* Where field `field` of every line lies.  D = the decoded data, nl = the one byte between lines, dl = the one byte
 * between fields, dl != nl.  Lines are numbered as for mi355x_bz2_line_hash: line k is closed by the k-th nl, counted from
 * 0; a non-empty unterminated tail is one more line, an empty one is none.  C = a line's content, without its nl, s = the
 * offset of its first byte.  parts = C split at every dl, as Python's bytes.split splits: the empty content has one field,
 * the empty one.  Field j, counted from 0, is present iff j < len( parts ); then start = s + sum( len( p ) + 1 for p in
 * parts[:j] ) and size = len( parts[j] ).  A missing field has start = s + len( C ) -- the offset of the closing nl, or of
 * the end of D for the tail -- and size = -1.  0 <= field <= 1023.  There is no quoting and no escaping: this is cut -f /
 * awk -F / bytes.split, not a CSV parser.
 *   _field_chunk_bytes  the bytes one GPU lane walks: of interest to tests and tuning.
 *   _field_spans      over spans as for _hash_lines (inside the last batch's output, no batch in flight).  dl == nl or
 *                     field > 1023 is MI355X_BZ2_ERR_INVALID_ARGUMENT, before anything is launched.  Per span i, read as
 *                     a stretch of D that a line may enter and leave, all positions relative to the span: count = the
 *                     lines it closes; has_delimiter; first_nl = its first nl (UINT64_MAX without one); head_delims = the
 *                     dl bytes in front of first_nl (in all of the span without an nl), saturated at field + 1, and
 *                     head_positions[i * ( field + 1 ) + k], k < head_delims, the position of the k-th of them (host
 *                     memory, room for n * ( field + 1 ); may be NULL); tail_start = the byte behind its last nl (0
 *                     without one); tail_delims = the dl bytes from there on, saturated at field + 1; tail_field_start,
 *                     tail_field_end = where the field of the line that begins at tail_start starts and ends,
 *                     UINT64_MAX where the span does not reach that; tail_non_empty = the span is not empty and its
 *                     last byte is not nl.  starts_device[] (uint64) and sizes_device[] (int64; both DEVICE memory, room
 *                     for `capacity`) receive start and size of the field in the closed lines, span by span in caller
 *                     order and in line order within a span, the first `capacity` of them, a start being an offset in
 *                     the batch's output; nothing is written at or beyond `capacity`.  The first closed line of a span
 *                     is computed as if the span were entered at a line start: the caller that knows the line's bytes
 *                     in front of the span replaces it (bz2_fields.hpp: stitchFields).  The call returns when
 *                     everything is written.  k_field_chunks, k_field_link, k_scan_tiles, k_field_emit, k_field_sizes. */
typedef struct mi355x_bz2_field_summary
{
    uint64_t count, first_nl, tail_start, tail_field_start, tail_field_end;
    uint32_t head_delims, tail_delims, has_delimiter, tail_non_empty;
} mi355x_bz2_field_summary;
uint32_t mi355x_bz2_field_chunk_bytes( void );
int mi355x_bz2_field_spans( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl,
                            uint32_t field, mi355x_bz2_field_summary* summaries, uint64_t* head_positions,
                            uint64_t* starts_device, int64_t* sizes_device, uint64_t capacity );

/* Field `field` of every line when fields may be quoted.  quote = one more byte, quote != nl and quote != dl.  Within a
 * line's content every quote byte toggles "inside quotes" and the content is parted at the dl bytes that lie OUTSIDE
 * quotes: a doubled quote inside a quoted field toggles twice and needs no rule of its own; an unbalanced quote makes
 * the rest of the line one field.  The nl always closes the line and resets the state: a quoted field cannot hold an nl,
 * and lines and their numbers are _field_spans'.  That parts the line into RAW fields; presence and "missing" are
 * _field_spans'.  The CONTENT of a raw field of 2 bytes or more whose first and last bytes are both quote is the raw
 * field without these two; any other raw field is its own content.  Doubled quotes inside stay doubled: spans of the
 * data are reported, no byte is rewritten.  No backslash escapes.
 *   _field_spans_quoted  _field_spans with these differences.  quote == nl or quote == dl is
 *                     MI355X_BZ2_ERR_INVALID_ARGUMENT, before anything is launched.  starts_device[] and sizes_device[]
 *                     receive CONTENT spans, the first closed line of a span computed as if the span were entered at a
 *                     line start outside quotes.  The summaries are RAW, not trimmed, and know both ways a span can be
 *                     entered: head_delims[h] and head_positions[( i * 2 + h ) * ( field + 1 ) + k], k < head_delims[h],
 *                     are the counted dl bytes in front of first_nl when the span is entered outside ( h = 0 ) and inside
 *                     ( h = 1 ) quotes (host memory, room for n * 2 * ( field + 1 ); may be NULL); head_quote_parity =
 *                     the parity of the quote bytes in front of first_nl (of all of them without an nl); the tail
 *                     members are those of a span entered outside quotes (behind an nl a line starts outside), and
 *                     tail_in_quote = the parity of the quote bytes from tail_start on.  bz2_fieldquote.hpp:
 *                     stitchQuotedFields.  k_field_chunks_quoted, k_field_link_quoted, k_scan_tiles,
 *                     k_field_emit_quoted, k_field_sizes, k_field_unquote. */
typedef struct mi355x_bz2_quoted_field_summary
{
    uint64_t count, first_nl, tail_start, tail_field_start, tail_field_end;
    uint32_t head_delims[2], tail_delims, has_delimiter, tail_non_empty, head_quote_parity, tail_in_quote, reserved;
} mi355x_bz2_quoted_field_summary;
int mi355x_bz2_field_spans_quoted( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl,
                                   uint8_t quote, uint32_t field, mi355x_bz2_quoted_field_summary* summaries,
                                   uint64_t* head_positions, uint64_t* starts_device, int64_t* sizes_device, uint64_t capacity );

/* A column of fields as bytes: the fields that _field_spans found, packed back to back in the order of their lines.
 *   _gather_fields_tile_bytes  the bytes of the destination one GPU workgroup writes: of interest to tests and tuning.
 *   _gather_fields    starts_device[n] (uint64) and sizes_device[n] (int64; both DEVICE memory) are n spans as
 *                     _field_spans writes them; `base` is what takes a start back to an offset in the last batch's
 *                     output: span i is its bytes [starts[i] - base, starts[i] - base + sizes[i]).  A span with a
 *                     size <= 0 (a missing or an empty field) has no bytes and its start does not matter.  The spans
 *                     may come in any order and may overlap.  offsets_device[n + 1] (uint64, DEVICE memory) receives
 *                     the exclusive prefix sums of max( size, 0 ), offsets[n] and *total their sum; the bytes of span
 *                     i go to dst_device[offsets[i], offsets[i + 1]) iff total <= dst_capacity and dst_device is not
 *                     NULL -- with NULL, or too little room, the call gives the total and the offsets, and writes
 *                     nothing to dst_device.  The GPU checks every span with bytes against the output's size before
 *                     any is read: with one that does not lie inside it the call is MI355X_BZ2_ERR_INVALID_ARGUMENT,
 *                     its message names the first such span, *total is 0, nothing is written to dst_device and what
 *                     offsets_device holds is not defined.  No batch may be in flight.  The call never reads outside
 *                     the batch's output and the slack behind it, and returns when everything is written.
 *                     k_fieldcol_sums, k_fieldcol_top, k_fieldcol_offsets, k_field_gather. */
uint32_t mi355x_bz2_gather_fields_tile_bytes( void );
int mi355x_bz2_gather_fields( mi355x_bz2_ctx* ctx, const uint64_t* starts_device, const int64_t* sizes_device, uint64_t n,
                              uint64_t base, uint64_t* offsets_device, void* dst_device, uint64_t dst_capacity,
                              uint64_t* total );

/* Is a field one of a set of values: the predicate of mi355x_bz2_reader_field_matches over columns that are in device
 * memory already.  A line MATCHES iff it has the field and the field's bytes are byte for byte one of the values; the
 * empty value matches an empty field that is present, never a missing one; equal values count once.  The key is only a
 * filter in front of the comparison of the bytes: the flags do not depend on `seed`, as long as the keys were made with it.
 *   _match_fields     `values` holds the n_values values one behind the other, value i with value_sizes[i] bytes: 1 to
 *                     1024 values of 0 to 256 bytes each and at most 16384 bytes in total.  keys_device[n] (uint64),
 *                     starts_device[n] (uint64) and sizes_device[n] (int64; all DEVICE memory) are what _field_hashes wrote
 *                     under `seed` for n lines of the last batch's output; `base` is what takes a start back to an offset
 *                     in that output, as for _gather_fields.  flags_device[n] (uint64, DEVICE memory) receives 1 for a
 *                     line that matches and 0 for every other; nothing is written at or beyond n.  A line with a size
 *                     < 0 (no such field) gives 0; so does one whose span does not lie inside the output, which is never
 *                     read.  The refusals come before anything is launched: a set outside the limits above, and two
 *                     DIFFERENT values with the same key under `seed` -- the message names both and says to pass another
 *                     seed --, MI355X_BZ2_ERR_INVALID_ARGUMENT; no batch may be in flight.  The call returns when
 *                     everything is written.  k_field_match. */
int mi355x_bz2_match_fields( mi355x_bz2_ctx* ctx, const uint8_t* values, const uint32_t* value_sizes, uint32_t n_values,
                             uint64_t seed, const uint64_t* keys_device, const uint64_t* starts_device,
                             const int64_t* sizes_device, uint64_t n, uint64_t base, uint64_t* flags_device );

/* Does a field match a regular expression: the predicate of mi355x_bz2_reader_field_matches_regex over columns that are in
 * device memory already.  The field is to the pattern what a line's content is to _match_lines: a line MATCHES iff it has
 * the field and the table of `re` (mi355x_bz2_regex_compile: its syntax, its refusals, its IGNORE_CASE flag), run from
 * state 0 over the field's bytes, reaches state 1 or ends in a state that accepts at the end.  `^` and `$` anchor to the
 * field's ends (awk '$3 ~ /^GET$/'); an empty field that is present matches iff state 0 accepts at the end; a missing
 * field never matches; a field may have any size.  For a field without the byte 0x0A this is Python's re.search( pattern,
 * field, re.DOTALL ); Python's `$` also matches in front of a trailing 0x0A, the table's does not.
 *   _match_fields_regex  starts_device[n] (uint64) and sizes_device[n] (int64; DEVICE memory) are what _field_spans wrote
 *                     for n lines of the last batch's output; `base` is what takes a start back to an offset in that
 *                     output, as for _gather_fields.  flags_device[n] (uint64, DEVICE memory) receives 1 for a line that
 *                     matches and 0 for every other; nothing is written at or beyond n.  A line with a size < 0 gives 0;
 *                     so does one whose span does not lie inside the output, which is never read.  No batch may be in
 *                     flight.  The call returns when everything is written.  k_field_regex: one lane per line, which
 *                     stops at the first byte after which the answer is known -- state 1, or the state from which no
 *                     match can follow --, so that an anchored prefix costs a few bytes per line. */
int mi355x_bz2_match_fields_regex( mi355x_bz2_ctx* ctx, const mi355x_bz2_regex* re, const uint64_t* starts_device,
                                   const int64_t* sizes_device, uint64_t n, uint64_t base, uint64_t* flags_device );

/* The hash of field `field` of every line: the KEY of a line is mi355x_bz2_line_hash's hash (same seed, same base) of
 * content.split( dl )[field], the field mi355x_bz2_field_spans finds; a line with fewer fields has the key
 * MI355X_BZ2_FIELD_MISSING = 2^61 - 1, the hash's modulus, which no hash takes; an empty field is present and hashes
 * to 0.  "Equal key" stands for "equal field" with the collision bound of mi355x_bz2_line_hash.
 *   _field_hashes     over spans as for _field_spans, with the same refusals before anything is launched.  Per span i,
 *                     summaries[i] holds _field_spans' summary, head_hash / head_xl / tail_hash / tail_xl as
 *                     _hash_lines' summary, and tail_start_hash, tail_end_hash = the hash of the bytes from tail_start up
 *                     to tail_field_start and to tail_field_end, where those are reached; head_hashes[i * ( field + 1 )
 *                     + k], k < head_delims, is the hash of the span's bytes in front of head_positions[...] (host
 *                     memory, room for n * ( field + 1 ) each; may be NULL).  hashes_device[] (uint64, DEVICE memory, room
 *                     for `capacity`) receives the keys of the closed lines in _field_spans' order, the first `capacity`
 *                     of them; starts_device[] and sizes_device[] receive what _field_spans writes, or are both NULL.
 *                     The first closed line of a span is computed as if the span were entered at a line start
 *                     (bz2_fieldhash.hpp: stitchFieldHashes).  The call returns when everything is written.
 *                     k_field_chunks, k_field_link, k_linehash_chunks, k_linehash_link, k_scan_tiles, k_fieldhash_emit,
 *                     k_fieldhash_finish. */
#define MI355X_BZ2_FIELD_MISSING 0x1FFFFFFFFFFFFFFFull
typedef struct mi355x_bz2_field_hash_summary
{
    uint64_t count, first_nl, tail_start, tail_field_start, tail_field_end;
    uint64_t head_hash, head_xl, tail_hash, tail_xl, tail_start_hash, tail_end_hash;
    uint32_t head_delims, tail_delims, has_delimiter, tail_non_empty;
} mi355x_bz2_field_hash_summary;
int mi355x_bz2_field_hashes( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl,
                             uint32_t field, uint64_t seed, mi355x_bz2_field_hash_summary* summaries, uint64_t* head_positions,
                             uint64_t* head_hashes, uint64_t* hashes_device, uint64_t* starts_device, int64_t* sizes_device,
                             uint64_t capacity );

/* Field `field` of every line as a number.  The bytes b of a field are a NUMBER iff they match [+-]?[0-9]{1,18} from end
 * to end, and the value is the decimal integer they spell: no whitespace, no '_', no hex, no floats; leading zeros count
 * towards the 18 digits; "-0" is 0; the empty field, "+", "-" and 19 or more digits are no numbers.  This is not awk's
 * strtod and not Python's int(), which both accept more.  18 digits always fit int64: nothing overflows, and a number has
 * at most 19 bytes.  Per line one int64 word: the value; MI355X_BZ2_FIELD_NOT_A_NUMBER = -2^63 where the field is present
 * and no number; MI355X_BZ2_FIELD_NUMBER_MISSING = -2^63 + 1 where the line has fewer fields.  No value takes either.
 * Fields and line numbering are those of mi355x_bz2_field_spans.
 *   _parse_field_number  the definition on the CPU: the value of bytes[0, size), or MI355X_BZ2_FIELD_NOT_A_NUMBER.
 *   _field_numbers    over spans as for _field_spans, with the same refusals before anything is launched and the same
 *                     summaries and head_positions.  A mi355x_bz2_field_text is the first 19 bytes of a byte string and
 *                     its size, saturated at 20.  head_texts[i * ( field + 1 ) + k], k <= head_delims and k <= field, is
 *                     that of span i's bytes between head position k - 1 (or the span's start) and head position k (or
 *                     first_nl, or the span's end); tail_texts[i] that of the field of the line that begins at
 *                     tail_start, from tail_field_start to tail_field_end or the span's end, empty where
 *                     tail_field_start is not reached (host memory, room for n * ( field + 1 ) and for n; each may be
 *                     NULL).  numbers_device[] (int64, DEVICE memory, room for `capacity`) receives the words of the
 *                     closed lines in _field_spans' order, the first `capacity` of them; starts_device[] and
 *                     sizes_device[] receive what _field_spans writes, or are both NULL.  Nothing is written at or
 *                     beyond `capacity`.  The first closed line of a span is computed as if the span were entered at a
 *                     line start: the caller that knows the field's bytes in front of the span replaces it
 *                     (bz2_fieldnum.hpp: stitchFieldNumbers).  The call returns when everything is written.
 *                     k_field_chunks, k_field_link, k_scan_tiles, k_field_emit, k_field_sizes, k_field_numbers,
 *                     k_field_texts. */
#define MI355X_BZ2_FIELD_NOT_A_NUMBER ( -0x7FFFFFFFFFFFFFFFll - 1 )
#define MI355X_BZ2_FIELD_NUMBER_MISSING ( -0x7FFFFFFFFFFFFFFFll )
typedef struct mi355x_bz2_field_text
{
    uint8_t size;
    uint8_t bytes[19];
} mi355x_bz2_field_text;
int64_t mi355x_bz2_parse_field_number( const uint8_t* bytes, uint64_t size );
int mi355x_bz2_field_numbers( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl,
                              uint32_t field, mi355x_bz2_field_summary* summaries, uint64_t* head_positions,
                              mi355x_bz2_field_text* head_texts, mi355x_bz2_field_text* tail_texts, int64_t* numbers_device,
                              uint64_t* starts_device, int64_t* sizes_device, uint64_t capacity );

/* Many independent bzip2 buffers (each a complete .bz2 byte string: ZIP members, Avro / Hadoop blocks, one blob per
 * sample) in shared GPU batches.  Buffer i decodes to exactly what mi355x_bz2_reader_open_memory( buffers[i], sizes[i],
 * 1, ... ) and a read to the end produce, stream-CRC check included; when that read would fail, results[i].status is
 * the status it fails with and error_offset_bits the bit offset (in the buffer) of the block or header where it does;
 * n_blocks and n_streams then count the blocks and streams that decoded in front of the failure (decoded_size is 0).
 * One bad buffer never fails the others; the return value is non-OK only for argument or device failures.
 * The buffers are copied (pageable memory is fine) in upload windows of up to 1 GiB, cut between buffers, into the
 * context's input: the call REPLACES the input made resident with mi355x_bz2_set_input_*, so a caller that also runs
 * decode_batch on this context sets its input again afterwards.  A window that does not fit on the device fails the call
 * with MI355X_BZ2_ERR_INVALID_ARGUMENT (a single buffer that large is for the reader, which streams).  Blocks are decoded in launches of at most max_launch_blocks (0 = 512; 10.1 MB of scratch per block), each
 * block bounded by its own buffer's end, so a damaged or truncated buffer reads none of its neighbour's bytes.
 * The output: buffer i's bytes are [output_offset, output_offset + decoded_size) of mi355x_bz2_output_device (read with
 * mi355x_bz2_copy_output / mi355x_bz2_gather_output; mi355x_bz2_copy_output_begin refuses it), in input order, back to
 * back; a failed buffer takes 0 bytes.  The
 * context keeps that buffer (grown, never shrunk) and it is valid until the next batch or call on the context.
 * *total_decoded = the sum of decoded_size.
 * One difference from the reader: a non-empty buffer that does not start with a stream header ("BZh1".."BZh9") fails
 * with MI355X_BZ2_ERR_STREAM_HEADER; the reader checks the header only once its magic scan has found a block, and reads
 * such bytes as an empty file if it finds none.  A 0-byte buffer decodes to 0 bytes, as in both.
 * Differences from CPython's bz2.decompress, which are the reader's:
 *   - bytes behind the last end-of-stream block that do not start a stream header are ignored and flagged in
 *     trailing_garbage (bz2.decompress raises OSError);
 *   - a stream header with no block magic behind it ("BZh9" alone) decodes to 0 bytes (bz2.decompress raises EOFError);
 *   - randomised blocks fail with MI355X_BZ2_ERR_RANDOMIZED (bz2.decompress decodes them).
 * No reference counterpart. */
typedef struct mi355x_bz2_buffer_result {
    uint64_t output_offset;      /* of this buffer's bytes in the context's output */
    uint64_t decoded_size;
    uint64_t error_offset_bits;  /* magic of the failing block, relative to the buffer (0 if OK) */
    uint32_t n_blocks, n_streams;
    int32_t  trailing_garbage;   /* bytes behind the last end-of-stream block were ignored */
    int32_t  status;             /* mi355x_bz2_status, as the reader would raise it for these bytes */
} mi355x_bz2_buffer_result;

int mi355x_bz2_decompress_buffers( mi355x_bz2_ctx* ctx, const uint8_t* const* buffers, const uint64_t* sizes,
                                   uint32_t n, uint32_t max_launch_blocks /* 0 = 512 */,
                                   mi355x_bz2_buffer_result* results, uint64_t* total_decoded );

/* bzip2 compression of many buffers (ZIP members, Avro / Hadoop blocks, one blob per sample) in shared GPU launches.
 * Buffer i becomes one complete single-stream .bz2 ("BZh<level>", its blocks, the end-of-stream block) that libbz2 and
 * this library decode back to exactly buffers[i]; an empty buffer becomes the 14-byte empty stream.  `level` 1..9 has
 * bzip2's meaning (blocks of 100k x level RLE1 bytes) and the blocks are cut exactly where libbz2 cuts them
 * (mi355x_bz2_plan_compress_blocks), so the block index matches that of libbz2's file of the same bytes; the encoded
 * bits may differ from libbz2's (Huffman tables are chosen independently; no randomised blocks).
 * Blocks of all buffers are encoded together in launches of at most max_launch_blocks (0 = 512) blocks and a device
 * memory budget (12 GiB; bz2_compress.hpp); a buffer whose blocks span several launches comes out byte-identical to one
 * compressed in a single launch.  Everything from RLE1 to bit packing runs in HIP kernels; the host only plans the
 * block cuts and places the blocks.  The outputs go back to back, in input order, into the context's result buffer:
 * buffer i is [output_offset, output_offset + compressed_size) of mi355x_bz2_output_device, read with
 * mi355x_bz2_copy_output or mi355x_bz2_gather_output (mi355x_bz2_copy_output_begin refuses it); valid until the next
 * batch or call on the context.  *total_compressed = the sum of compressed_size.  The encoder's device scratch is
 * allocated by the first call and kept (mi355x_bz2_encoder_memory); the decoder's scratch does not change.  Returns
 * MI355X_BZ2_ERR_INVALID_ARGUMENT for a level outside 1..9.  No reference counterpart (the reference only decodes). */
typedef struct mi355x_bz2_compress_result {
    uint64_t output_offset;      /* of this buffer's stream in the context's output */
    uint64_t compressed_size;    /* bytes */
    uint64_t map_first;          /* where this buffer's entries start in the block map of the call */
    uint32_t n_blocks;           /* data blocks */
    uint32_t map_entries;        /* entries of its block map (mi355x_bz2_compress_block_map) */
    int32_t  status;             /* mi355x_bz2_status */
    int32_t  reserved;
} mi355x_bz2_compress_result;

int mi355x_bz2_compress_buffers( mi355x_bz2_ctx* ctx, const uint8_t* const* buffers, const uint64_t* sizes, uint32_t n,
                                 int level, uint32_t max_launch_blocks /* 0 = 512 */,
                                 mi355x_bz2_compress_result* results, uint64_t* total_compressed );

/* The block map of buffer `buffer` of the last compress call: what mi355x_bz2_reader_block_offsets returns for its
 * output (bit offsets in the buffer's stream, decoded byte offsets): every data block, the end-of-stream block and the
 * end of the file -- {0: 0} for an empty buffer.  *count = the number of entries; at most `capacity` are written.
 * Ready for mi355x_bz2_reader_set_block_offsets. */
int mi355x_bz2_compress_block_map( mi355x_bz2_ctx* ctx, uint32_t buffer, uint64_t* bit_offsets, uint64_t* byte_offsets,
                                   uint64_t capacity, uint64_t* count );

/* Device bytes of the encoder's scratch (0 until the context's first compress call). */
int mi355x_bz2_encoder_memory( mi355x_bz2_ctx* ctx, uint64_t* bytes );

/* Host only, no GPU: the input sizes of the blocks libbz2 cuts `size` bytes into at `level` (RLE1 pieces -- runs of one
 * byte cut every 255 bytes, L < 4 bytes taking L RLE1 bytes, L >= 4 taking 5 -- and a block ending with the first piece
 * that brings its RLE1 size to 100000 x level - 19 or more).  *count = the number of blocks; at most `capacity` sizes
 * are written. */
int mi355x_bz2_plan_compress_blocks( const uint8_t* data, uint64_t size, int level, uint64_t* block_sizes,
                                     uint64_t capacity, uint64_t* count );

/* ------------------------------------------------------------------------------------------------ 2. magic scan */

#define MI355X_BZ2_MAGIC_BLOCK 0x314159265359ULL   /* bzip2.hpp:103 */
#define MI355X_BZ2_MAGIC_EOS   0x177245385090ULL   /* bzip2.hpp:104 */

/* All bit offsets (ascending) at which the 48-bit pattern occurs in bytes[0,size).  Returns the number found; at most
 * `capacity` are written.  `threads` = 0 picks the host's core count.
 * Replaces ParallelBitStringFinder<48>::find (src/core/ParallelBitStringFinder.hpp:159-265). */
uint64_t mi355x_bz2_find_magic( const uint8_t* bytes, uint64_t size, uint64_t magic48,
                                uint64_t* bit_offsets, uint64_t capacity, uint32_t threads );

/* The same scan on the GPU over the input made resident with mi355x_bz2_set_input_* (ascending offsets; at most
 * `capacity` are written, *n_found = number of matches).  At GPU decode rates the host scan would otherwise be the
 * critical path. */
int mi355x_bz2_find_magic_device( mi355x_bz2_ctx* ctx, uint64_t magic48, uint64_t* bit_offsets, uint64_t capacity,
                                  uint64_t* n_found );

/* bzip2::readBzip2Header (bzip2.hpp:114-142) at a byte-aligned bit offset: returns level 1..9, or 0 if invalid. */
int mi355x_bz2_read_stream_header( const uint8_t* bytes, uint64_t size, uint64_t bit_offset );

/* ------------------------------------------------------------------------------------------------ 3. reader */

typedef struct mi355x_bz2_reader mi355x_bz2_reader;

/* ParallelBZ2Reader( filePath | fd | memory, parallelization )    ParallelBZ2Reader.hpp:50-89
 * parallelization = number of blocks kept in flight per GPU batch (0 = default). */
int mi355x_bz2_reader_open_path( const char* path, uint32_t parallelization, int32_t device, mi355x_bz2_reader** r );
int mi355x_bz2_reader_open_fd( int fd, uint32_t parallelization, int32_t device, mi355x_bz2_reader** r );
int mi355x_bz2_reader_open_memory( const uint8_t* bytes, uint64_t size, uint32_t parallelization, int32_t device,
                                   mi355x_bz2_reader** r );
void mi355x_bz2_reader_close( mi355x_bz2_reader* r );                        /* close()        :104-111 */
const char* mi355x_bz2_reader_last_error( const mi355x_bz2_reader* r );

/* read( fd, buffer, n ): writes to `fd` if fd >= 0, else copies to `buffer` if non-NULL, else discards
 * (BZ2ReaderInterface.hpp:35-57 + ParallelBZ2Reader.hpp:167-269).  *n_read = bytes produced. */
int mi355x_bz2_reader_read( mi355x_bz2_reader* r, int fd, void* buffer, uint64_t n_bytes, uint64_t* n_read );
/* seek( offset, whence ) with SEEK_SET/SEEK_CUR/SEEK_END          ParallelBZ2Reader.hpp:271-325 */
int mi355x_bz2_reader_seek( mi355x_bz2_reader* r, int64_t offset, int whence, uint64_t* new_position );
uint64_t mi355x_bz2_reader_tell( const mi355x_bz2_reader* r );                /* tell()         :129-142 */
int      mi355x_bz2_reader_eof( const mi355x_bz2_reader* r );                 /* eof()          :119-123 */
int      mi355x_bz2_reader_closed( const mi355x_bz2_reader* r );              /* closed()       :113-117 */
/* size(): returns 1 and *size if the block map is finalized, else 0             :144-151 */
int      mi355x_bz2_reader_size( const mi355x_bz2_reader* r, uint64_t* size );
uint64_t mi355x_bz2_reader_tell_compressed( const mi355x_bz2_reader* r );     /* tellCompressed :385-393 */
int      mi355x_bz2_reader_block_offsets_complete( const mi355x_bz2_reader* r ); /*             :329-333 */

/* pread of many ranges at once: range i is [offsets[i], offsets[i] + sizes[i]) of the decoded file, and its bytes go to
 * dst + sizes[0] + ... + sizes[i - 1]; n_read[i] = bytes produced (short only at the end of the file; the bytes of dst
 * behind them are not written).  Every block that some range needs is decoded once, in launches of at most
 * `parallelization` blocks, and only the requested bytes are copied out of HBM (k_gather).  dst_is_device: dst is device
 * memory on the reader's device.  Does not move the read position or eof(); ranges behind the indexed part of the file
 * are indexed first, as a forward seek would.  A block that fails to decode fails the call with its status (dst is then
 * unspecified).  No reference counterpart (ParallelBZ2Reader reads one range at a time). */
int mi355x_bz2_reader_read_ranges( mi355x_bz2_reader* r, const uint64_t* offsets, const uint64_t* sizes, uint32_t n,
                                   void* dst, int dst_is_device, uint64_t* n_read );

/* ---- line access.  D = the decoded file, `nl` = one delimiter byte (any value: '\n', '\r', 0).  N = the number of nl
 * bytes in D.  Line k (0-based) starts at s(k): s(0) = 0, s(k) = 1 + the position of the k-th nl (1 <= k <= N); line N
 * is the unterminated tail D[s(N):], possibly empty.  The line range (first, count) is D[s(first) : s(first + count)]
 * (closing nl included) if first + count <= N, D[s(first):] if first <= N < first + count, and nothing if first > N or
 * count == 0: the readLines loop of rapidgzip (src/tools/rapidgzip.cpp:624-748) -- the reference has line access for
 * gzip only, not for bzip2.
 * The line index has one entry per data block plus the end: {decoded offset of the block's first byte -> nl bytes in
 * front of it}, ..., {size of D -> N}; {0 -> 0} for an empty file (rapidgzip's m_newlineOffsets: one NewlineOffset per
 * chunk and the final one, ParallelGzipReader.hpp:90, 1056-1145).  The reader keeps one index, together with its nl; a
 * line function called with another nl, or before any index exists, builds it first.
 * All of these are positionless like read_ranges: tell(), eof() and the sequential reader's decoded runs stay as they
 * are, the launches go to the front of the queue and decode at most `parallelization` blocks each. */

/* The line index for `nl`, built if the reader does not hold it: the block map is completed first if it is not (as
 * block_offsets does), then every data block is decoded once and k_count_byte counts nl in it; nothing but the counts
 * leaves the GPU.  Two-call protocol as block_offsets: capacity 0 gives the count in *n. */
int mi355x_bz2_reader_line_offsets( mi355x_bz2_reader* r, uint8_t nl, uint64_t* bytes, uint64_t* lines,
                                    uint64_t capacity, uint64_t* n );
/* Import of a line index for `nl`.  Needs a complete block map (MI355X_BZ2_ERR_INVALID_ARGUMENT otherwise, and when the
 * keys are not exactly the data blocks' decoded offsets plus the size, the values do not start at 0 or decrease, or a
 * block is given more delimiters than it has bytes).  An index that fits the map but not the data is found out when a
 * line is looked for: that call fails with MI355X_BZ2_ERR_LOGIC. */
int mi355x_bz2_reader_set_line_offsets( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* bytes, const uint64_t* lines,
                                        uint64_t n );
/* byte_offsets[i] = s( lines[i] ), or the size of D for lines[i] > N.  Decodes only the blocks that hold one of the
 * delimiters asked for (k_find_byte finds them); no data byte is copied out. */
int mi355x_bz2_reader_line_starts( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* lines, uint32_t n,
                                   uint64_t* byte_offsets );
/* Many line ranges at once, in two steps, because nobody knows a range's size before its blocks are decoded (compare
 * mi355x_bz2_decompress_buffers followed by mi355x_bz2_copy_output / _gather_output).
 * Step 1, _read_line_ranges: every block some range needs -- from the block that holds the first-th delimiter through
 * the one that holds the (first + count)-th, or the last block -- is decoded once, k_find_byte resolves the ranges' ends
 * in the decoded blocks, and k_gather packs each launch's pieces into a buffer of the context that ran it, where they
 * are held.  byte_sizes[i] = the bytes of range i, *total their sum.  keep_on_device tells where step 2 will write
 * (1: device memory); it is recorded for the check in step 2 and moves no data.
 * Step 2, _take_line_ranges: writes range i at dst + byte_sizes[0] + ... + byte_sizes[i - 1] (dst_is_device must equal
 * keep_on_device; for a host destination exactly the requested bytes cross to the host, for a device destination none)
 * and releases what step 1 held.  The next line call, or close, releases it as well.
 * A block that fails to decode fails step 1 with its status and bit offset. */
int mi355x_bz2_reader_read_line_ranges( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* first, const uint64_t* count,
                                        uint32_t n, int keep_on_device, uint64_t* byte_sizes, uint64_t* total );
int mi355x_bz2_reader_take_line_ranges( mi355x_bz2_reader* r, void* dst, int dst_is_device );

/* ---- search.  D = the decoded file, P = `pattern`, m = pattern_size with 1 <= m <= 256 (the slack behind the output
 * buffers, and what keeps the bytes a launch hands the host for its seams under 512); m == 0 or m > 256 is
 * MI355X_BZ2_ERR_INVALID_ARGUMENT.  A match is every offset p with D[p : p + m] == P, start <= p and p + m <= end, where
 * start and end are clipped to [0, size of D]; an empty range, or one shorter than m, has none.  Matches that overlap
 * themselves all count: "abab" in "abababab" matches at 0, 2 and 4 (bytes.count of Python says 2).
 * Positionless like read_ranges and the line functions: tell(), eof(), the sequential reader's decoded runs and the held
 * line ranges stay as they are, the launches go to the front of the queue and decode at most `parallelization` blocks
 * each (0 = 512), and a part of the file in front of `end` that is not indexed yet is indexed first.  Every data block
 * that intersects [start, end) is decoded once per call; k_count_bytes / k_emit_bytes find the matches inside a launch's
 * part of the range, and the matches that straddle two or more launches are found on the host from the first and last
 * m - 1 bytes of each part (bz2_search.hpp).  Nothing but counts, positions and those seam bytes leaves the GPU.  A
 * block that fails to decode fails the call with its status and bit offset.  No reference counterpart.
 * Two steps, as for line ranges, because nobody knows the number of matches in advance.
 * Step 1, _search.  limit == 0: count only -- *n_matches is the number of matches in the range, nothing is held and no
 * emitting pass runs.  limit > 0 (UINT64_MAX: all): the first min( limit, total ) positions, ascending, are held on the
 * host and *n_matches is their number; no launch is started after the one in which the limit was reached (launches
 * already taken by a context finish).
 * Step 2, _take_matches: copies the held positions (at most `capacity`) and releases them; the next search, or close,
 * releases them as well.  Held matches and held line ranges are independent.
 * _search_ex is _search with `flags` (MI355X_BZ2_SEARCH_*; _search is flags 0).  An unknown bit is
 * MI355X_BZ2_ERR_INVALID_ARGUMENT, named by _last_error, before anything is launched or held.  With
 * MI355X_BZ2_SEARCH_IGNORE_CASE a match is every p with fold( D[p + j] ) == fold( P[j] ) for all j < m, fold( b ) =
 * b | 0x20 for 'A' <= b <= 'Z' and b otherwise; the range rule, overlaps and the limit are unchanged, the same launches
 * run, and the seam bytes are folded on the host. */
int mi355x_bz2_reader_search( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t pattern_size, uint64_t start,
                              uint64_t end, uint64_t limit, uint64_t* n_matches );
int mi355x_bz2_reader_search_ex( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t pattern_size, uint32_t flags,
                                 uint64_t start, uint64_t end, uint64_t limit, uint64_t* n_matches );
int mi355x_bz2_reader_take_matches( mi355x_bz2_reader* r, uint64_t* positions, uint64_t capacity );

/* ---- grep and line numbers: the line functions and the search joined.  D, nl, N and s(k) as under line access.
 * L(p) = the number of nl bytes in D[0 : min( p, size )]: the 0-based line that holds byte p, s( L(p) ) <= p <
 * s( L(p) + 1 ) for p < size (with s(N + 1) read as the size); L(p) = N for every p at or beyond the size, and 0 for every
 * p of an empty file.  Positionless like the line functions, and built on the same line index (built first if the reader
 * does not hold one for nl). */

/* lines[i] = L( offsets[i] ), the inverse of _line_starts; the offsets come in any order, repeats included.  Decodes only
 * the blocks that hold an offset which is not their first byte (the index answers that one, and everything at or beyond
 * the size); k_rank_byte counts the delimiters in front of the offsets, one pass over a 64-KiB tile however many offsets
 * fall into it, and only the counts leave the GPU.  An imported index that does not fit the data of a decoded block
 * fails the call with MI355X_BZ2_ERR_LOGIC.  Releases held line ranges, as every line call does. */
int mi355x_bz2_reader_line_numbers( mi355x_bz2_reader* r, uint8_t nl, const uint64_t* offsets, uint64_t n, uint64_t* lines );
/* The lines that hold a match (bzgrep -F, grep -n).  The matches are exactly those of _search for (pattern, start, end):
 * 1 <= pattern_size <= 256 (else, or with a null pattern, MI355X_BZ2_ERR_INVALID_ARGUMENT before anything is launched),
 * overlapping matches included, start and end bound the matches and not the lines.  A match belongs to the line of its
 * FIRST byte (the pattern may contain nl).  A matching line is a line with at least one match: each is reported once, in
 * ascending order, whole and with its delimiter -- also where it reaches outside [start, end) --, the unterminated tail
 * as it is.
 * Step 1, _grep.  max_lines == 0: count only -- *n_lines is the number of distinct matching lines, nothing is held.
 * Otherwise the first min( max_lines, all ) matching lines are held as by _read_line_ranges with one range (line, 1)
 * each, *n_lines is their number and *total_bytes the sum of their sizes; keep_on_device as there.  Three passes: the
 * search over the whole of [start, end) whatever max_lines is, the rank pass of _line_numbers over the blocks that hold
 * a match's first byte (decoded a second time: the passes share nothing), and the line ranges.  Matches and line ranges
 * held by earlier calls are released.
 * Step 2, _take_grep: the numbers and byte sizes of the held lines (at most `capacity`); the bytes stay held.  With
 * nothing held: MI355X_BZ2_ERR_INVALID_ARGUMENT.
 * Step 3, the bytes: _take_line_ranges, which releases everything.
 * _grep_ex passes `flags` to its search pass (the matches are those of _search_ex); the rank and line passes do not
 * depend on them. */
int mi355x_bz2_reader_grep( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t pattern_size, uint8_t nl, uint64_t start,
                            uint64_t end, uint64_t max_lines, int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );
int mi355x_bz2_reader_grep_ex( mi355x_bz2_reader* r, const uint8_t* pattern, uint32_t pattern_size, uint32_t flags, uint8_t nl,
                               uint64_t start, uint64_t end, uint64_t max_lines, int keep_on_device, uint64_t* n_lines,
                               uint64_t* total_bytes );
int mi355x_bz2_reader_take_grep( mi355x_bz2_reader* r, uint64_t* line_numbers, uint64_t* byte_sizes, uint64_t capacity );

/* ---- search and grep for a set of patterns: what `grep -F -f FILE` does, with ONE decode of every block of the range
 * whatever the number of patterns.  The set as for mi355x_bz2_count_bytes_set (patterns concatenated in set order; 1 to
 * 1024 patterns of 1 to 256 bytes, 16384 bytes in total, else MI355X_BZ2_ERR_INVALID_ARGUMENT before anything is launched,
 * the limit named by _last_error).  A match is a pair (p, i) with D[p : p + m_i] == pattern i, start <= p and
 * p + m_i <= end, start and end clipped as for _search and the end rule applied per pattern; the matches of pattern i are
 * exactly those of _search for it, overlapping ones included.  A result is ordered by ascending p, then ascending i.
 * Positionless, same launches, residency and failure rules as _search; the pairs that straddle launches are found on the
 * host from the first and last m_max - 1 bytes of each launch's part (bz2_search.hpp).
 * Step 1, _search_set.  limit == 0: count only -- *n_matches is the number of pairs and per_pattern[i] (may be NULL) the
 * count of pattern i, nothing is held.  limit > 0 (UINT64_MAX: all): the first min( limit, total ) pairs are held on the
 * host, *n_matches is their number and per_pattern is not written.  The result with a limit is the first `limit` pairs
 * of the result without one; the launches behind the front are skipped only once the front holds `limit` pairs that end
 * m_max bytes in front of its end (a long pattern that crosses the front's end may sort in front of a short one inside).
 * Step 2, _take_set_matches: copies the held pairs (at most `capacity`) and releases them; the next set search, or
 * close, releases them as well.  Held set matches are independent of held single-pattern matches and of held line
 * ranges.
 * _search_set_ex and _grep_set_ex take the flags of _search_ex, checked with the set before anything is launched. */
int mi355x_bz2_reader_search_set( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* pattern_sizes,
                                  uint32_t n_patterns, uint64_t start, uint64_t end, uint64_t limit, uint64_t* n_matches,
                                  uint64_t* per_pattern );
int mi355x_bz2_reader_search_set_ex( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* pattern_sizes,
                                     uint32_t n_patterns, uint32_t flags, uint64_t start, uint64_t end, uint64_t limit,
                                     uint64_t* n_matches, uint64_t* per_pattern );
int mi355x_bz2_reader_take_set_matches( mi355x_bz2_reader* r, uint64_t* positions, uint32_t* ids, uint64_t capacity );
/* _grep with the set search as its first pass: a matching line is a line that holds the first byte of at least one pair,
 * each reported once (the positions are deduplicated before the rank pass).  _take_grep and _take_line_ranges serve it
 * unchanged. */
int mi355x_bz2_reader_grep_set( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* pattern_sizes,
                                uint32_t n_patterns, uint8_t nl, uint64_t start, uint64_t end, uint64_t max_lines,
                                int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );
int mi355x_bz2_reader_grep_set_ex( mi355x_bz2_reader* r, const uint8_t* patterns, const uint32_t* pattern_sizes,
                                   uint32_t n_patterns, uint32_t flags, uint8_t nl, uint64_t start, uint64_t end,
                                   uint64_t max_lines, int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );

/* ---- grep for a regular expression (bzgrep PATTERN, grep -n): _grep with a DFA run as its first pass.  `re` comes from
 * mi355x_bz2_regex_compile, which also says which lines match.  The whole file is searched: there is no start / end.
 * The launches are those of _search over [0, size); each runs mi355x_bz2_match_lines on its part on the context that
 * decoded it, the host composes the parts' summaries (lines that cross launches, `^` and `$` included) into one offset per
 * matching line, and the rank and line passes of _grep follow.  max_lines == 0 counts only: no emitting pass, no rank
 * pass, nothing held.  Otherwise the first min( max_lines, all ) matching lines are held; _take_grep and
 * _take_line_ranges serve them unchanged.  Positionless; holds and releases as _grep does, same failure rules. */
int mi355x_bz2_reader_grep_regex( mi355x_bz2_reader* r, const mi355x_bz2_regex* re, uint8_t nl, uint64_t max_lines,
                                  int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );

/* ---- line hashes (mi355x_bz2_line_hash says what the hash of a line is, and how lines are numbered).
 *   _line_hashes      the hashes of lines [first, first + count), count clipped at the last line; *n_lines = their number.
 *                     Needs the line index for `nl` (built on first use, as _read_line_ranges).  Only the blocks that hold
 *                     those lines are decoded, each once, in the launches of _read_line_ranges for the range (first,
 *                     count), with its residency and failure rules; each launch hashes its blocks on the context that
 *                     decoded them (mi355x_bz2_hash_lines' kernels) straight into one device buffer of the reader's, and
 *                     the host stitches the launches' summaries and patches the one line per launch that crosses a seam.
 *                     The buffer is allocated before anything is launched: a failed allocation is
 *                     MI355X_BZ2_ERR_DEVICE with a message.  The hashes are held until the next _line_hashes or
 *                     _distinct_lines or the close.  Positionless; releases line ranges held by earlier calls.
 *   _take_line_hashes the first min( capacity, n_lines ) held hashes (uint64 each) to `dst`, host memory or, with
 *                     dst_is_device, device memory; they stay held.
 *   _line_hashes_device  the held hashes on the GPU (uint64[n_lines]; NULL if none are held or keep_on_device was 0);
 *                     valid until the next _line_hashes or _distinct_lines or the close.
 *   _distinct_lines   *n_distinct = the number of distinct hashes among all lines of the file.  The hashes of the whole
 *                     file go into one device buffer as for _line_hashes( 0, all ); a stable radix sort (rocPRIM) of
 *                     (hash, line number) over 61 bits, a flag on the first element of every run of equal hashes, and
 *                     their count.  With want_numbers != 0 the flagged line numbers are selected and sorted ascending:
 *                     the first occurrence of every distinct line (awk '!seen[$0]++'), held for _take_distinct_lines.
 *                     Every device buffer is allocated before the pass that fills it; a failed allocation is
 *                     MI355X_BZ2_ERR_DEVICE with a message.  Nothing of _line_hashes stays held.
 *   _take_distinct_lines  the first min( capacity, n_distinct ) held line numbers, ascending; they stay held until the
 *                     next _distinct_lines, _line_hashes or the close. */
int mi355x_bz2_reader_line_hashes( mi355x_bz2_reader* r, uint8_t nl, uint64_t seed, uint64_t first, uint64_t count,
                                   int keep_on_device, uint64_t* n_lines );
int mi355x_bz2_reader_take_line_hashes( mi355x_bz2_reader* r, void* dst, uint64_t capacity, int dst_is_device );
const uint64_t* mi355x_bz2_reader_line_hashes_device( mi355x_bz2_reader* r );
int mi355x_bz2_reader_distinct_lines( mi355x_bz2_reader* r, uint8_t nl, uint64_t seed, int want_numbers, uint64_t* n_distinct );
int mi355x_bz2_reader_take_distinct_lines( mi355x_bz2_reader* r, uint64_t* line_numbers, uint64_t capacity );

/* ---- fields (mi355x_bz2_field_spans says what field j of a line is, and how lines are numbered).
 *   _field_spans      where field `field` lies in lines [first, first + count), count clipped at the last line; *n_lines =
 *                     their number.  dl == nl or field > 1023 is MI355X_BZ2_ERR_INVALID_ARGUMENT, before anything is
 *                     launched.  Needs the line index for `nl` (built on first use, as _read_line_ranges).  Only the
 *                     blocks that hold those lines are decoded, each once, in the launches of _line_hashes for the same
 *                     range, with their residency and failure rules; each launch runs mi355x_bz2_field_spans' kernels on
 *                     the context that decoded its blocks, straight into two device buffers of the reader's, and the host
 *                     stitches the launches' summaries and patches the one line per launch that crosses a seam, and the
 *                     tail.  The buffers are allocated before anything is launched: a failed allocation is
 *                     MI355X_BZ2_ERR_DEVICE with a message.  The spans are held until the next _field_spans or the
 *                     close.  Positionless; releases line ranges held by earlier calls.
 *   _take_field_spans the first min( capacity, n_lines ) held starts (uint64 each, offsets in the decoded file) and sizes
 *                     (int64 each, -1 for a missing field) to `starts` and `sizes`, host memory or, with dst_is_device,
 *                     device memory; they stay held. */
int mi355x_bz2_reader_field_spans( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count,
                                   int keep_on_device, uint64_t* n_lines );
int mi355x_bz2_reader_take_field_spans( mi355x_bz2_reader* r, void* starts, void* sizes, uint64_t capacity, int dst_is_device );

/* ---- field columns: the bytes of several fields of every line, each packed in line order, from one decode.
 *   _field_columns    for lines [first, first + count), count clipped at the last line, and each of the n_fields (1 to 16)
 *                     entries of `fields` (each at most 1023; one may be named twice, every entry gets a column of its
 *                     own): the bytes of that field of every line back to back, the n_lines + 1 offsets of the lines'
 *                     fields in them and the n_lines sizes, -1 where a line has no such field, which then owns no bytes.
 *                     *n_lines = the lines, total_bytes[i] = the bytes of column i.  n_fields 0 or above 16, a field
 *                     above 1023 and dl == nl are MI355X_BZ2_ERR_INVALID_ARGUMENT, before anything is launched.  The
 *                     launches are _field_spans' for the same range; every launch runs _field_spans' kernels once per
 *                     field over its resident blocks and mi355x_bz2_gather_fields' into a buffer of its own per field,
 *                     allocated when its size is known: every needed block is decoded ONCE per call, whatever the number
 *                     of fields.  The host stitches the summaries per field; the one line per launch that crosses a seam,
 *                     and the tail, are fetched as byte ranges (_read_ranges' path): the few blocks that hold them are
 *                     the only ones decoded a second time.  The final offsets are scanned on the device; nothing per
 *                     line passes through the host.  Peak device memory: the columns' bytes once and 24 bytes per line
 *                     and field.  A failed allocation is MI355X_BZ2_ERR_DEVICE with a message, and nothing stays held.
 *                     The columns are held, as the launches' pieces, until the next _field_columns or the close.
 *                     Positionless; releases line ranges held by earlier calls, and nothing else.
 *   _take_field_column  held column `column` (an index into `fields`): its bytes assembled straight into `data`
 *                     (total_bytes[column] bytes), its offsets (uint64, n_lines + 1) and sizes (int64, n_lines), each to
 *                     host memory or, with dst_is_device, device memory, each skipped if NULL; the column stays held. */
int mi355x_bz2_reader_field_columns( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, const uint32_t* fields, uint32_t n_fields,
                                     uint64_t first, uint64_t count, int keep_on_device, uint64_t* n_lines,
                                     uint64_t* total_bytes );
int mi355x_bz2_reader_take_field_column( mi355x_bz2_reader* r, uint32_t column, void* data, void* offsets, void* sizes,
                                         int dst_is_device );

/* ---- quoted fields (mi355x_bz2_field_spans_quoted says what a quoted field is: every quote byte toggles, a dl inside
 * quotes does not part, the nl always closes the line, the content loses its enclosing pair, doubled quotes stay doubled).
 *   _field_spans_quoted    _field_spans with the CONTENT of the fields under `quote`; quote == nl or quote == dl is
 *                     MI355X_BZ2_ERR_INVALID_ARGUMENT, before anything is launched.  Each launch runs
 *                     mi355x_bz2_field_spans_quoted's kernels.  The lines the host patches -- one per launch seam, and
 *                     the tail -- come out of the stitcher raw: the first and last byte of each that has 2 bytes or more
 *                     are fetched in ONE call of _read_ranges' path, and the pair is taken off on the host.  Held and
 *                     taken as _field_spans' result: _take_field_spans serves both.
 *   _field_columns_quoted  _field_columns likewise, its fix-ups trimmed the same way before the offsets are scanned;
 *                     _take_field_column serves both. */
int mi355x_bz2_reader_field_spans_quoted( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first,
                                          uint64_t count, int keep_on_device, uint64_t* n_lines, uint8_t quote );
int mi355x_bz2_reader_field_columns_quoted( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, const uint32_t* fields, uint32_t n_fields,
                                            uint64_t first, uint64_t count, int keep_on_device, uint64_t* n_lines,
                                            uint64_t* total_bytes, uint8_t quote );

/* ---- field hashes and groups (mi355x_bz2_field_hashes says what the key of a line is).
 *   _field_hashes     the keys of lines [first, first + count), count clipped at the last line; *n_lines = their number.
 *                     Refusals, line index, launches, residency and failure rules are _field_spans': every needed block
 *                     is decoded once per call, each launch runs mi355x_bz2_field_hashes' kernels on the context that
 *                     decoded its blocks, straight into three device buffers of the reader's (keys, starts, sizes)
 *                     allocated before anything is launched, and the host stitches the launches' summaries and patches
 *                     one key and one span per seam and for the tail.  Keys and spans are held until the next
 *                     _field_hashes or _field_groups or the close.  Positionless; releases line ranges held by earlier
 *                     calls.
 *   _take_field_hashes  the first min( capacity, n_lines ) held keys (uint64 each) to `dst`, host memory or, with
 *                     dst_is_device, device memory; they stay held.
 *   _field_groups     the lines [first, first + count) grouped by key: _field_hashes, then on the GPU a stable radix sort
 *                     (rocPRIM) of (key, line) over 61 bits, a flag on the first element of every run, the run starts
 *                     selected, and per run its length, its first line and that line's field span; the run of
 *                     MI355X_BZ2_FIELD_MISSING is dropped and its length is *n_missing; the others, *n_groups of them,
 *                     are sorted by first line.  32 bytes per group come to the host and nothing per line.  Nothing of
 *                     _field_hashes stays held; the groups are held until the next call of this family or the close.
 *   _take_field_groups  of the first min( capacity, n_groups ) held groups, ascending by first line: lines[] = the first
 *                     line (numbered in the file), counts[] = the number of lines with that key, starts[] / sizes[] = the
 *                     field in that first line.  Any of the four may be NULL. */
int mi355x_bz2_reader_field_hashes( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first,
                                    uint64_t count, int keep_on_device, uint64_t* n_lines );
int mi355x_bz2_reader_take_field_hashes( mi355x_bz2_reader* r, void* dst, uint64_t capacity, int dst_is_device );
int mi355x_bz2_reader_field_groups( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t seed, uint64_t first,
                                    uint64_t count, uint64_t* n_groups, uint64_t* n_missing );
int mi355x_bz2_reader_take_field_groups( mi355x_bz2_reader* r, uint64_t* lines, uint64_t* counts, uint64_t* starts,
                                         int64_t* sizes, uint64_t capacity );

/* ---- field numbers and sums (mi355x_bz2_field_numbers says what the number of a field is: not awk's strtod).
 *   _field_numbers    the int64 words of lines [first, first + count), count clipped at the last line; *n_lines = their
 *                     number.  Refusals, line index, launches, residency and failure rules are _field_spans': every needed
 *                     block is decoded once per call, each launch runs mi355x_bz2_field_numbers' kernels on the context
 *                     that decoded its blocks, straight into three device buffers of the reader's (numbers, starts,
 *                     sizes) allocated before anything is launched, and the host stitches the launches' summaries and
 *                     patches one number and one span per seam and for the tail.  They are held until the next
 *                     _field_numbers or _field_sums or the close.  Positionless; releases line ranges held by earlier
 *                     calls.
 *   _take_field_numbers  the first min( capacity, n_lines ) held words (int64 each) to `dst`, host memory or, with
 *                     dst_is_device, device memory; they stay held.
 *   _field_sums       the lines [first, first + count) grouped by the key of key_field (mi355x_bz2_field_hashes' key
 *                     under `seed`), with the numbers of value_field summed per group: every needed block is decoded
 *                     ONCE, each launch runs the field-hash kernels for key_field and the field-number kernels for
 *                     value_field over the same resident bytes; then on the GPU a stable radix sort (rocPRIM) of (key,
 *                     line) over 61 bits and one reduce-by-key over the values in that order -- a 128-bit sum, min, max,
 *                     the count of numbers, the count of lines and the first line --, so that one key shared by every
 *                     line costs what all-distinct keys cost.  The run of MI355X_BZ2_FIELD_MISSING is dropped and its
 *                     length is *n_missing; the others, *n_groups of them, are sorted by first line.  72 bytes per group
 *                     come to the host and nothing per line.  key_field == value_field is allowed.  Nothing per line
 *                     stays held; the groups are held until the next call of this family or the close.
 *   _take_field_sums  of the first min( capacity, n_groups ) held groups, ascending by first line: lines[] = the first
 *                     line (numbered in the file), counts[] = the lines with that key, starts[] / sizes[] = the key
 *                     field in that first line, numbers[] = those of the lines whose value field is a number, sums_lo[]
 *                     (uint64) and sums_hi[] (int64) their exact sum = hi * 2^64 + lo, mins[] / maxs[] the least and the
 *                     largest of them, MI355X_BZ2_FIELD_NOT_A_NUMBER where numbers[] is 0.  Any of the nine may be
 *                     NULL. */
int mi355x_bz2_reader_field_numbers( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, uint64_t first, uint64_t count,
                                     int keep_on_device, uint64_t* n_lines );
int mi355x_bz2_reader_take_field_numbers( mi355x_bz2_reader* r, void* dst, uint64_t capacity, int dst_is_device );
int mi355x_bz2_reader_field_sums( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t key_field, uint32_t value_field,
                                  uint64_t seed, uint64_t first, uint64_t count, uint64_t* n_groups, uint64_t* n_missing );
int mi355x_bz2_reader_take_field_sums( mi355x_bz2_reader* r, uint64_t* lines, uint64_t* counts, uint64_t* starts, int64_t* sizes,
                                       uint64_t* numbers, uint64_t* sums_lo, int64_t* sums_hi, int64_t* mins, int64_t* maxs,
                                       uint64_t capacity );

/* ---- lines selected by a field (mi355x_bz2_match_fields says when a field is one of a set of values;
 * mi355x_bz2_field_numbers what the number of a field is).  A predicate on field `field` is a set of VALUES or a RANGE
 * lo <= n <= hi over the field's number: a field that is no number and a line without the field are in no range.  A side
 * without has_lo / has_hi is open; bounds are clipped to [-(10^18 - 1), 10^18 - 1], the numbers there are, and lo > hi
 * afterwards is the empty range, not an error.  With `invert` the complement within the line range is selected (grep -v):
 * then also the lines without the field and, for a range, the fields that are no numbers.  Lines, fields, first / count
 * and line numbers are _field_spans'; there is no quoting, this is not a CSV parser.
 *   _field_matches    the lines of [first, first + count), count clipped at the last line, whose field is one of the
 *                     values (limits and refusals of mi355x_bz2_match_fields, which come before anything is decoded).
 *                     *n_matching (may be NULL) = their number, *n_selected = min( limit, *n_matching ): the first
 *                     n_selected line numbers, ascending and numbered in the file, are held in device memory until the
 *                     next _field_matches / _field_in_range / _select_lines or the close.  limit 0 counts: nothing per
 *                     line leaves the GPU, 8 bytes come to the host.  Every needed block is decoded ONCE: each launch runs
 *                     mi355x_bz2_field_hashes' kernels and k_field_match over its resident blocks, then one rocPRIM select
 *                     over the flags.  A line that crosses a launch seam and the unterminated tail are known by key, start
 *                     and size only: where key and size hit a value, the field's bytes are fetched by one
 *                     _read_ranges-like call -- at most launches + 1 fields, the only second decode -- and compared on
 *                     the host.  The answer does not depend on `seed`.  Line index, launches, residency and failure rules
 *                     are _field_spans'.  Positionless; releases line ranges held by earlier calls.
 *   _field_in_range   the same for a range: mi355x_bz2_reader_field_numbers' launches, then the select over the numbers.
 *   _take_field_matches  the first min( capacity, n_selected ) held line numbers (uint64 each) to `dst`, host memory or,
 *                     with dst_is_device, device memory; they stay held.
 *   _select_lines     the selected lines themselves: values (n_values > 0) or a range (n_values == 0), not both; then
 *                     _read_line_ranges with one range per selected line, as _grep does it.  max_lines is grep's: 0 gives
 *                     *n_lines = the number of selected lines and holds nothing; otherwise the first max_lines lines are
 *                     held as grep's: _take_grep gives their numbers and sizes, _take_line_ranges their bytes. */
int mi355x_bz2_reader_field_matches( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const uint8_t* values,
                                     const uint32_t* value_sizes, uint32_t n_values, uint64_t seed, int invert, uint64_t first,
                                     uint64_t count, uint64_t limit, int keep_on_device, uint64_t* n_selected,
                                     uint64_t* n_matching );
int mi355x_bz2_reader_field_in_range( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, int has_lo, int64_t lo,
                                      int has_hi, int64_t hi, int invert, uint64_t first, uint64_t count, uint64_t limit,
                                      int keep_on_device, uint64_t* n_selected, uint64_t* n_matching );
int mi355x_bz2_reader_take_field_matches( mi355x_bz2_reader* r, void* dst, uint64_t capacity, int dst_is_device );
int mi355x_bz2_reader_select_lines( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field, const uint8_t* values,
                                    const uint32_t* value_sizes, uint32_t n_values, uint64_t seed, int has_lo, int64_t lo,
                                    int has_hi, int64_t hi, int invert, uint64_t first, uint64_t count, uint64_t max_lines,
                                    int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );

/* ---- lines selected by a regular expression on a field (mi355x_bz2_match_fields_regex says when a field matches): a
 * third predicate beside the values and the range above, with the same `invert`, the same line range and the same holds.
 *   _field_matches_regex  as _field_matches, with `re` (mi355x_bz2_regex_compile; a pattern it refuses never gets here) in
 *                     place of the values: each launch runs mi355x_bz2_field_spans' kernels and k_field_regex over its
 *                     resident blocks, every needed block decoded ONCE, then one rocPRIM select over the flags.  A line
 *                     that crosses a launch seam and the unterminated tail are known by start and size only: an empty
 *                     field is decided at once, the bytes of the others are fetched by one _read_ranges-like call -- at
 *                     most launches + 1 fields, the only second decode -- and the table is run on the host.  The line
 *                     numbers are held as _field_matches holds them: _take_field_matches gives them, and the next
 *                     _field_matches / _field_in_range / _field_matches_regex / _select_lines(_regex) releases them.
 *   _select_lines_regex  as _select_lines: the result is held as grep's, _take_grep + _take_line_ranges. */
int mi355x_bz2_reader_field_matches_regex( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field,
                                           const mi355x_bz2_regex* re, int invert, uint64_t first, uint64_t count,
                                           uint64_t limit, int keep_on_device, uint64_t* n_selected, uint64_t* n_matching );
int mi355x_bz2_reader_select_lines_regex( mi355x_bz2_reader* r, uint8_t nl, uint8_t dl, uint32_t field,
                                          const mi355x_bz2_regex* re, int invert, uint64_t first, uint64_t count,
                                          uint64_t max_lines, int keep_on_device, uint64_t* n_lines, uint64_t* total_bytes );

/* blockOffsets() (forces a full decode) / availableBlockOffsets(): two-call protocol -- pass capacity 0 to get the
 * count in *n, then call again with arrays of that size.                         :339-363 */
int mi355x_bz2_reader_block_offsets( mi355x_bz2_reader* r, uint64_t* bits, uint64_t* bytes, uint64_t capacity,
                                     uint64_t* n );
int mi355x_bz2_reader_available_block_offsets( const mi355x_bz2_reader* r, uint64_t* bits, uint64_t* bytes,
                                               uint64_t capacity, uint64_t* n );
/* setBlockOffsets( map )                                                       :365-378 */
int mi355x_bz2_reader_set_block_offsets( mi355x_bz2_reader* r, const uint64_t* bits, const uint64_t* bytes,
                                         uint64_t n );
/* joinThreads()                                                                :404-409 */
int mi355x_bz2_reader_join_threads( mi355x_bz2_reader* r );

/* Check of the combined CRC in every end-of-stream block against the block CRCs decoded in front of it
 * (crc = rotl( crc, 1 ) ^ blockCRC, BZ2Reader.hpp:481-484; a mismatch fails the read with MI355X_BZ2_ERR_STREAM_CRC as
 * BZ2Reader.hpp:406-416 throws).  The reference only does this in its serial reader, which is what parallelization
 * == 1 selects there; ParallelBZ2Reader never checks.  Same default here: on for parallelization == 1, else off.
 * The check covers streams whose blocks are decoded for the first time in order, i.e. not after set_block_offsets. */
int mi355x_bz2_reader_set_verify_stream_crc( mi355x_bz2_reader* r, int enable );
/* number of end-of-stream CRCs that have been compared (and matched) so far */
uint64_t mi355x_bz2_reader_streams_verified( const mi355x_bz2_reader* r );

/* BlockFetcher::Statistics subset (src/core/BlockFetcher.hpp:52-173) */
typedef struct mi355x_bz2_reader_stats {
    uint64_t gets, cache_hits, prefetch_hits, on_demand_fetches, prefetches_submitted, batches, blocks_decoded;
    uint64_t failed_prefetches;
    double   decode_seconds, wait_seconds;
    /* (ABI 2) 1: the whole compressed file is kept on the GPU; 0: bounded residency -- the file does not fit beside the
     * decoders' scratch, or exceeds MI355X_BZ2_INPUT_BUDGET bytes (environment), and every launch copies the byte range of
     * its own blocks (the reference streams through 128 KiB refills, src/core/BitReader.hpp:57) */
    uint64_t input_resident;
    uint64_t input_bytes_uploaded;   /* bounded residency: compressed bytes copied to the GPU so far, all launches */
} mi355x_bz2_reader_stats;
int mi355x_bz2_reader_statistics( const mi355x_bz2_reader* r, mi355x_bz2_reader_stats* stats );

/* ------------------------------------------------------------------------------------------------ 4. chunk decoding */

/* Counterpart of rapidgzip's bzip2 chunk decoder, Bzip2Chunk<ChunkData>::decodeChunk
 * (src/rapidgzip/chunkdecoding/Bzip2Chunk.hpp:215-268) and decodeUnknownBzip2Chunk (:34-212): decodes the run of
 * consecutive blocks that starts at chunk_offset_bits -- or, if nothing decodes there, at the first block magic behind it
 * that does -- through end-of-stream blocks and the headers of following streams, up to (excluding) the first block that
 * starts at or behind until_offset_bits, or until max_decoded_bytes have been produced (stopped_preemptively).
 * `bytes` is the host view of the input that was given to mi355x_bz2_set_input_* (magic scan and headers are read on the
 * host, all blocks of the range are decoded in ONE GPU batch).  The chunk's bytes are
 * [data_offset, data_offset + decoded_size) of mi355x_bz2_output_device / mi355x_bz2_copy_output.
 * blocks[k] (k < n_blocks): the records of the chunk's data blocks, data_offset relative to the chunk -- the
 * {encoded offset, decoded offset} pairs are what ChunkData::appendDeflateBlockBoundary receives; footers[k]: the position
 * behind every end-of-stream block and the decoded size so far (ChunkData::appendFooter).
 * result->status: MI355X_BZ2_OK or MI355X_BZ2_ERR_NO_BLOCK_IN_RANGE (the reference throws NoBlockInRange). */
typedef struct mi355x_bz2_chunk_boundary {
    uint64_t encoded_offset_bits;
    uint64_t decoded_offset;
} mi355x_bz2_chunk_boundary;

typedef struct mi355x_bz2_chunk_result {
    uint64_t encoded_offset_bits;   /* where the chunk really starts */
    uint64_t encoded_end_bits;      /* ChunkData::finalize( nextBlockOffset ) */
    uint64_t decoded_size;
    uint64_t data_offset;           /* of the chunk in the context's output buffer */
    uint32_t n_blocks;
    uint32_t n_footers;
    int32_t  stopped_preemptively;
    int32_t  status;
} mi355x_bz2_chunk_result;

int mi355x_bz2_decode_chunk( mi355x_bz2_ctx* ctx, const uint8_t* bytes, uint64_t size,
                             uint64_t chunk_offset_bits, uint64_t until_offset_bits, uint64_t max_decoded_bytes,
                             mi355x_bz2_chunk_result* result,
                             mi355x_bz2_block_result* blocks, uint32_t blocks_capacity,
                             mi355x_bz2_chunk_boundary* footers, uint32_t footers_capacity );

#ifdef __cplusplus
}
#endif
#endif /* MI355X_BZ2_H */
