/**
 * bz2_ctx.hpp -- entry points of the decoder context that other host code of the library uses but the C ABI does not
 * export: the batch, its buffers and the encoder's slot (bz2_device.hip), the reader's one-span forms of the calls that
 * read a batch's output (bz2_queries.hip.h, in the same translation unit), and device memory of nobody's context
 * (bz2_distinct.hip).
 */
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/mi355x_bz2.h"
#include "bz2_fieldhash.hpp"
#include "bz2_fieldmatch.hpp"
#include "bz2_fieldregex.hpp"
#include "bz2_fieldnum.hpp"
#include "bz2_fieldquote.hpp"
#include "bz2_fields.hpp"
#include "bz2_linehash.hpp"
#include "bz2_regex.hpp"
#include "bz2_search.hpp"

/** What mi355x_bz2_regex_compile hands out (bz2_regex.cpp). */
struct mi355x_bz2_regex
{
    bz2gpu::Regex dfa;
};

namespace mi355x
{
/** mi355x_bz2_decode_batch_begin with an optional end of the input per block: the scan kernels read block i's bits only
 * up to min( input size, endBytes[i] ) bytes, as if the input ended there.  nullptr: the whole input (the public form). */
int decodeBatchBegin( mi355x_bz2_ctx* ctx, const uint64_t* offsets, const uint64_t* endBytes, uint32_t n );

/** A context-owned device buffer of at least `size` bytes, grown (its first `keep` bytes copied along) and kept across
 * calls. */
int resultBuffer( mi355x_bz2_ctx* ctx, uint64_t size, uint64_t keep, uint8_t** device );

/** mi355x_bz2_gather_output with the result buffer as the source: pieces [src_offset, src_offset + size) of it go to
 * `dst`.  Unlike the public call it may run while a batch is in flight on the context (the result buffer is not a batch
 * output); the kernel then queues behind what that batch has put on the context's stream. */
int gatherResult( mi355x_bz2_ctx* ctx, const mi355x_bz2_gather_piece* pieces, uint32_t nPieces, void* dst, int dstIsDevice );

/** The reader's search in one launch: the matches of `pattern` (m bytes) inside `extent` of the last batch's output,
 * as mi355x_bz2_find_bytes with that one span.  *count is the true count; with `positions` given it is resized to the
 * first min( *count, limit ) offsets in the output (nullptr: count only, no emitting pass).  The first and the last
 * min( m - 1, extent.size ) bytes of the extent come back in the same D2H as the count: seamBytes[0, ...) and
 * seamBytes[256, ...) of a 512-byte array, raw whatever the flags.  `flags`: MI355X_BZ2_SEARCH_*. */
int searchOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, const uint8_t* pattern, uint32_t m, uint32_t flags,
                  uint64_t limit, std::vector<uint64_t>* positions, uint64_t* count, uint8_t* seamBytes );

/** searchOutput for a set of patterns (as mi355x_bz2_find_bytes_set with that one span): *count is the true number of
 * pairs; with `positions` and `ids` given they are resized to the first min( *count, limit ) pairs in (position, id) order
 * (both nullptr: count only).  perPattern (may be nullptr) receives the count of every pattern inside the extent.  The
 * first and the last min( m_max - 1, extent.size ) bytes of the extent come back as searchOutput hands them over.  The
 * set carries the one flag there is: makePatternSet's fold. */
int searchOutputSet( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, const bz2gpu::PatternSet& set, uint64_t limit,
                     std::vector<uint64_t>* positions, std::vector<uint32_t>* ids, uint64_t* count, uint64_t* perPattern,
                     uint8_t* seamBytes );

/** The reader's regular-expression pass in one launch: mi355x_bz2_match_lines with `extent` as its one span.  *summary
 * receives the extent's summary and the true count of its body witnesses; with limit > 0 its witnesses are the first
 * min( count, limit ) of them as offsets in the output (0: count only, no emitting pass). */
int matchLinesOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, const bz2gpu::Regex& regex, uint8_t nl,
                      uint64_t limit, bz2gpu::StretchSummary* summary );

/** The reader's hashing pass in one launch: mi355x_bz2_hash_lines with `extent` as its one span and the base x instead of
 * the seed.  *summary receives the extent's summary and the count of the lines it closes, no hashes; the hashes of its
 * closed lines [skip, skip + take) go to dHashes[0, ...), device memory (take 0: no emitting pass). */
int hashLinesOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, uint8_t nl, uint64_t x, uint64_t skip, uint64_t take,
                     uint64_t* dHashes, bz2gpu::HashSummary* summary );

/** The reader's field pass in one launch: mi355x_bz2_field_spans with `extent` as its one span, whose first byte is
 * offset `fileOffset` of the decoded file.  *summary receives the extent's summary for `field` and the count of the
 * lines it closes, none of them listed; start and size of the field in its closed lines [skip, skip + take) go to
 * dStarts[0, ...) and dSizes[0, ...), device memory, the starts as offsets in the file. */
int fieldSpansOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                      uint32_t field, uint64_t skip, uint64_t take, uint64_t* dStarts, int64_t* dSizes, bz2gpu::FieldSummary* summary );

/** fieldSpansOutput under a quote: mi355x_bz2_field_spans_quoted with `extent` as its one span.  dStarts and dSizes receive
 * the fields' contents; *summary is raw and knows both entry hypotheses (bz2_fieldquote.hpp). */
int fieldSpansQuotedOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                            uint8_t quote, uint32_t field, uint64_t skip, uint64_t take, uint64_t* dStarts, int64_t* dSizes,
                            bz2gpu::QuotedFieldSummary* summary );

/** The reader's gather in one launch: mi355x_bz2_gather_fields over the n spans that fieldSpansOutput wrote for an extent
 * that begins at `srcOffset` of the last batch's output and at `fileOffset` of the decoded file.  When the total is known,
 * allocate( total ) names the device memory the bytes go to (not called for a total of 0; nullptr: there is none, and the
 * call is MI355X_BZ2_ERR_DEVICE with a message).  dOffsets[0, n] receives the offsets, *firstSize the bytes of span 0. */
int gatherFieldsOutput( mi355x_bz2_ctx* ctx, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n, uint64_t srcOffset,
                        uint64_t fileOffset, uint64_t* dOffsets, const std::function<uint8_t*( uint64_t )>& allocate,
                        uint64_t* total, uint64_t* firstSize );

/** The reader's field-hash pass in one launch: mi355x_bz2_field_hashes with `extent` as its one span, whose first byte is
 * offset `fileOffset` of the decoded file, and the base x instead of the seed.  *summary receives the extent's summary
 * and the count of the lines it closes, none of them listed; key, start and size of the field in its closed lines [skip,
 * skip + take) go to dKeys[0, ...), dStarts[0, ...) and dSizes[0, ...), device memory, the starts as offsets in the file. */
int fieldHashesOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                       uint32_t field, uint64_t x, uint64_t skip, uint64_t take, uint64_t* dKeys, uint64_t* dStarts, int64_t* dSizes,
                       bz2gpu::FieldHashSummary* summary );

/** The reader's field-number pass in one launch: mi355x_bz2_field_numbers with `extent` as its one span, whose first byte
 * is offset `fileOffset` of the decoded file.  *summary receives the extent's summary with its texts and the count of the
 * lines it closes, none of them listed; the number of the field in its closed lines [skip, skip + take) goes to
 * dNumbers[0, ...), device memory, and start and size to dStarts[0, ...) and dSizes[0, ...), the starts as offsets in the
 * file, unless both are null. */
int fieldNumbersOutput( mi355x_bz2_ctx* ctx, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                        uint32_t field, uint64_t skip, uint64_t take, int64_t* dNumbers, uint64_t* dStarts, int64_t* dSizes,
                        bz2gpu::FieldNumberSummary* summary );

/** The reader's value match in one launch: mi355x_bz2_match_fields with a finished table, over the n lines whose keys,
 * starts and sizes fieldHashesOutput wrote for an extent that begins at `srcOffset` of the last batch's output and at
 * `fileOffset` of the decoded file.  dFlags[0, n), device memory, receives 1 where the field's bytes are one of the table's
 * values and 0 elsewhere. */
int matchFieldsOutput( mi355x_bz2_ctx* ctx, const bz2gpu::ValueTable& table, const uint64_t* dKeys, const uint64_t* dStarts,
                       const int64_t* dSizes, uint64_t n, uint64_t srcOffset, uint64_t fileOffset, uint64_t* dFlags );

/** The reader's regular-expression match on a field in one launch: mi355x_bz2_match_fields_regex over the n lines whose
 * starts and sizes fieldSpansOutput wrote for an extent that begins at `srcOffset` of the last batch's output and at
 * `fileOffset` of the decoded file.  dFlags[0, n), device memory, receives 1 where the field matches (bz2_fieldregex.hpp)
 * and 0 elsewhere. */
int matchFieldsRegexOutput( mi355x_bz2_ctx* ctx, const bz2gpu::Regex& regex, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n,
                            uint64_t srcOffset, uint64_t fileOffset, uint64_t* dFlags );

/** Device memory that is nobody's context's (bz2_distinct.hip): the reader's line hashes.  device < 0: the current one.
 * allocate returns nullptr with *error set.  The copies wait for their completion; deviceToHost with dstIsDevice copies
 * to device memory instead. */
void* deviceAllocate( int device, uint64_t bytes, std::string* error );
void deviceRelease( void* pointer );
bool deviceToHost( int device, void* dst, const void* src, uint64_t bytes, bool dstIsDevice, std::string* error );
bool hostToDevice( int device, void* dst, const void* src, uint64_t bytes, std::string* error );

/** dOffsets[0, n] = the exclusive prefix sums of max( dSizes[i], 0 ) (both device memory; rocPRIM, bz2_distinct.hip) and
 * *total their sum.  False with *error set if an allocation or a launch fails. */
bool columnOffsets( int device, const int64_t* dSizes, uint64_t n, uint64_t* dOffsets, uint64_t* total, std::string* error );

/** The distinct values among dHashes[0, n) (device memory, left as it is): *nDistinct = their number and, if `numbers` is
 * given, the index of the first occurrence of each, ascending.  False with *error set if an allocation or a launch
 * fails; every buffer is allocated before the pass that fills it. */
bool distinctHashes( int device, const uint64_t* dHashes, uint64_t n, uint64_t* nDistinct, std::vector<uint64_t>* numbers,
                     std::string* error );

/** One group of lines with the same key: its first line, its size, and the field in that first line. */
struct FieldGroup
{
    uint64_t line{ 0 }, count{ 0 }, start{ 0 };
    int64_t size{ 0 };
};

/** The lines 0 .. n - 1 grouped by dKeys[0, n), with dStarts / dSizes their fields (device memory, left as it is):
 * *groups = one FieldGroup per distinct key but `missing`, ascending by first line; *nMissing = the lines with the key
 * `missing`.  False with *error set if an allocation or a launch fails; every buffer is allocated before the pass that
 * fills it. */
bool groupHashes( int device, const uint64_t* dKeys, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n, uint64_t missing,
                  std::vector<FieldGroup>* groups, uint64_t* nMissing, std::string* error );

/** One group of lines with the same key and the numbers among their values: the FieldGroup, how many of the values are
 * numbers, their exact sum = sumHi * 2^64 + sumLo, and the least and the largest of them (FIELD_NOT_A_NUMBER without
 * one). */
struct FieldSumGroup
{
    uint64_t line{ 0 }, count{ 0 }, start{ 0 };
    int64_t size{ 0 };
    uint64_t numbers{ 0 }, sumLo{ 0 };
    int64_t sumHi{ 0 }, min{ 0 }, max{ 0 };
};

/** groupHashes with dValues[0, n), the lines' field-number words, reduced per group in one reduce-by-key behind the
 * sort: a key that every line shares costs what all-distinct keys cost. */
bool groupSums( int device, const uint64_t* dKeys, const uint64_t* dStarts, const int64_t* dSizes, const int64_t* dValues, uint64_t n,
                uint64_t missing, std::vector<FieldSumGroup>* groups, uint64_t* nMissing, std::string* error );

/** What selectLines selects by: dFlags[i] != 0 (one word per line), or, with dFlags null, lo <= dNumbers[i] <= hi over
 * field-number words, whose two sentinels lie below every lo there is.  `invert` selects the others. */
struct LinePredicate
{
    const uint64_t* dFlags{ nullptr };
    const int64_t* dNumbers{ nullptr };
    int64_t lo{ 0 }, hi{ 0 };
    bool invert{ false };
};

/** The numbers base + i, ascending, of the i < n for which the predicate holds (device memory, left as it is; rocPRIM
 * select over a counting iterator): *nMatching = how many there are, which takes 8 bytes to the host, and *selected = new
 * device memory (deviceRelease) with the first min( limit, *nMatching ) of them, null where that is none.  False with
 * *error set if an allocation or a launch fails. */
bool selectLines( int device, const LinePredicate& predicate, uint64_t n, uint64_t base, uint64_t limit, uint64_t** selected,
                  uint64_t* nMatching, std::string* error );

/** From now until the next batch begins, mi355x_bz2_output_device / _copy_output / _gather_output address the first
 * `size` bytes of the result buffer. */
int publishResult( mi355x_bz2_ctx* ctx, uint64_t size );

/** The encoder state slot of the context (nullptr until the first mi355x_bz2_compress_buffers); `release` frees what
 * it holds when the context is destroyed. */
void*& encoderOf( mi355x_bz2_ctx* ctx, void ( *release )( void* ) );

/** The device ordinal the context was created on. */
int deviceOf( const mi355x_bz2_ctx* ctx );

/** Bytes of the larger of the context's own input copies (reused by the next mi355x_bz2_set_input_host). */
uint64_t inputCapacity( const mi355x_bz2_ctx* ctx );

/** What mi355x_bz2_last_error returns from now on. */
void setLastError( mi355x_bz2_ctx* ctx, const std::string& message );
}  // namespace mi355x
