"""ctypes binding of the C ABI declared in include/mi355x_bz2.h (libmi355x_bz2.so, built by build.py).

The product path has no CPU fallback: if the HIP library is missing or no MI355X is present, the functions here
raise -- nothing in this package imports or calls oracle/.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MI355X_BZ2_LIBRARY: development only, an A/B build of the same ABI)
LIB_PATH = os.environ.get("MI355X_BZ2_LIBRARY") or os.path.join(_HERE, "libmi355x_bz2.so")

MAGIC_BLOCK = 0x314159265359
MAGIC_EOS = 0x177245385090

OK = 0
ERR_CRC = 15
ERR_STREAM_CRC = 17
ERR_NO_DEVICE = 102
ERR_INVALID_ARGUMENT = 103


class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("max_batch_blocks", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BlockResult(ctypes.Structure):
    _fields_ = [
        ("encoded_offset_bits", ctypes.c_uint64),
        ("encoded_size_bits", ctypes.c_uint64),
        ("decoded_size", ctypes.c_uint64),
        ("data_offset", ctypes.c_uint64),
        ("header_crc", ctypes.c_uint32),
        ("computed_crc", ctypes.c_uint32),
        ("bwt_length", ctypes.c_uint32),
        ("orig_ptr", ctypes.c_uint32),
        ("n_symbols", ctypes.c_uint32),
        ("is_eos", ctypes.c_int32),
        ("is_eof", ctypes.c_int32),
        ("status", ctypes.c_int32),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


MAX_KERNELS = 16


class Timings(ctypes.Structure):
    _fields_ = [("ms_total", ctypes.c_float), ("ms_kernel_sum", ctypes.c_float), ("n_kernels", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("ms_kernel", ctypes.c_float * MAX_KERNELS)]

    def as_dict(self):
        names = [lib().mi355x_bz2_kernel_name(i).decode() for i in range(self.n_kernels)]
        return {"ms_total": self.ms_total, "ms_kernel_sum": self.ms_kernel_sum,
                "kernels": {names[i]: self.ms_kernel[i] for i in range(self.n_kernels)}}


class ChunkBoundary(ctypes.Structure):
    _fields_ = [("encoded_offset_bits", ctypes.c_uint64), ("decoded_offset", ctypes.c_uint64)]


class ChunkResult(ctypes.Structure):
    _fields_ = [("encoded_offset_bits", ctypes.c_uint64), ("encoded_end_bits", ctypes.c_uint64),
                ("decoded_size", ctypes.c_uint64), ("data_offset", ctypes.c_uint64),
                ("n_blocks", ctypes.c_uint32), ("n_footers", ctypes.c_uint32),
                ("stopped_preemptively", ctypes.c_int32), ("status", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ReaderStats(ctypes.Structure):
    _fields_ = [("gets", ctypes.c_uint64), ("cache_hits", ctypes.c_uint64), ("prefetch_hits", ctypes.c_uint64),
                ("on_demand_fetches", ctypes.c_uint64), ("prefetches_submitted", ctypes.c_uint64),
                ("batches", ctypes.c_uint64), ("blocks_decoded", ctypes.c_uint64),
                ("failed_prefetches", ctypes.c_uint64),
                ("decode_seconds", ctypes.c_double), ("wait_seconds", ctypes.c_double),
                ("input_resident", ctypes.c_uint64), ("input_bytes_uploaded", ctypes.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class GatherPiece(ctypes.Structure):
    _fields_ = [("src_offset", ctypes.c_uint64), ("dst_offset", ctypes.c_uint64), ("size", ctypes.c_uint64)]


class ByteSpan(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint64)]


class ByteQuery(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint64), ("rank", ctypes.c_uint64)]


class RankQuery(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint64), ("position", ctypes.c_uint64)]


class BufferResult(ctypes.Structure):
    _fields_ = [("output_offset", ctypes.c_uint64), ("decoded_size", ctypes.c_uint64),
                ("error_offset_bits", ctypes.c_uint64), ("n_blocks", ctypes.c_uint32), ("n_streams", ctypes.c_uint32),
                ("trailing_garbage", ctypes.c_int32), ("status", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class CompressResult(ctypes.Structure):
    _fields_ = [("output_offset", ctypes.c_uint64), ("compressed_size", ctypes.c_uint64),
                ("map_first", ctypes.c_uint64), ("n_blocks", ctypes.c_uint32), ("map_entries", ctypes.c_uint32),
                ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


# every symbol include/mi355x_bz2.h declares: (name, restype, argtypes)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_vp = ctypes.c_void_p
SYMBOLS = [
    ("mi355x_bz2_status_string", ctypes.c_char_p, [ctypes.c_int]),
    ("mi355x_bz2_abi_version", ctypes.c_int, []),
    ("mi355x_bz2_create", ctypes.c_int, [ctypes.POINTER(Config), ctypes.POINTER(_vp)]),
    ("mi355x_bz2_warmup", ctypes.c_int, [ctypes.c_int32]),
    ("mi355x_bz2_destroy", None, [_vp]),
    ("mi355x_bz2_last_error", ctypes.c_char_p, [_vp]),
    ("mi355x_bz2_set_input_host", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint64]),
    ("mi355x_bz2_set_input_host_async", ctypes.c_int, [_vp, ctypes.c_void_p, ctypes.c_uint64]),
    ("mi355x_bz2_set_input_host_streamed", ctypes.c_int, [_vp, ctypes.c_void_p, ctypes.c_uint64]),
    ("mi355x_bz2_input_resident", ctypes.c_int, [_vp]),
    ("mi355x_bz2_set_input_device", ctypes.c_int, [_vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_decode_batch", ctypes.c_int, [_vp, _u64p, ctypes.c_uint32, ctypes.POINTER(BlockResult), _u64p]),
    ("mi355x_bz2_decode_batch_begin", ctypes.c_int, [_vp, _u64p, ctypes.c_uint32]),
    ("mi355x_bz2_decode_batch_end", ctypes.c_int, [_vp, ctypes.POINTER(BlockResult), _u64p]),
    ("mi355x_bz2_output_device", _vp, [_vp]),
    ("mi355x_bz2_copy_output", ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
    ("mi355x_bz2_copy_output_begin", ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
    ("mi355x_bz2_copy_output_end", ctypes.c_int, [_vp]),
    ("mi355x_bz2_hold_output_until", ctypes.c_int, [_vp, _vp]),
    ("mi355x_bz2_last_timings", ctypes.c_int, [_vp, ctypes.POINTER(Timings)]),
    ("mi355x_bz2_last_pipeline_ms", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    ("mi355x_bz2_kernel_name", ctypes.c_char_p, [ctypes.c_uint32]),
    ("mi355x_bz2_stream", _vp, [_vp]),
    ("mi355x_bz2_device_memory", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    ("mi355x_bz2_debug_copy_stage", ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_int, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_find_magic", ctypes.c_uint64, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, _u64p,
                                                 ctypes.c_uint64, ctypes.c_uint32]),
    ("mi355x_bz2_share_input", ctypes.c_int, [_vp, _vp]),
    ("mi355x_bz2_find_magic_device", ctypes.c_int, [_vp, ctypes.c_uint64, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_crc32_device", ctypes.c_int, [_vp, _vp, _u64p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    ("mi355x_bz2_gather_output", ctypes.c_int, [_vp, ctypes.POINTER(GatherPiece), ctypes.c_uint32, _vp, ctypes.c_int]),
    ("mi355x_bz2_count_byte", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, _u64p]),
    ("mi355x_bz2_find_byte", ctypes.c_int, [_vp, ctypes.POINTER(ByteQuery), ctypes.c_uint32, ctypes.c_uint8, _u64p]),
    ("mi355x_bz2_rank_byte", ctypes.c_int, [_vp, ctypes.POINTER(RankQuery), ctypes.c_uint32, ctypes.c_uint8, _u64p]),
    ("mi355x_bz2_count_bytes", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p,
                                               ctypes.c_uint32, _u64p]),
    ("mi355x_bz2_find_bytes", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p,
                                              ctypes.c_uint32, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_count_bytes_set", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p, _u32p,
                                                   ctypes.c_uint32, _u64p, _u64p]),
    ("mi355x_bz2_find_bytes_set", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p, _u32p,
                                                  ctypes.c_uint32, _u64p, _u32p, ctypes.c_uint64, _u64p, _u64p]),
    ("mi355x_bz2_count_bytes_ex", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p,
                                                  ctypes.c_uint32, ctypes.c_uint32, _u64p]),
    ("mi355x_bz2_find_bytes_ex", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p,
                                                 ctypes.c_uint32, ctypes.c_uint32, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_count_bytes_set_ex", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p, _u32p,
                                                      ctypes.c_uint32, ctypes.c_uint32, _u64p, _u64p]),
    ("mi355x_bz2_find_bytes_set_ex", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_char_p, _u32p,
                                                     ctypes.c_uint32, ctypes.c_uint32, _u64p, _u32p, ctypes.c_uint64, _u64p,
                                                     _u64p]),
    ("mi355x_bz2_regex_compile", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(_vp),
                                                 ctypes.c_char_p, ctypes.c_uint64]),
    ("mi355x_bz2_regex_free", None, [_vp]),
    ("mi355x_bz2_regex_states", ctypes.c_uint32, [_vp]),
    ("mi355x_bz2_regex_table", ctypes.c_int, [_vp, _vp, _vp]),
    ("mi355x_bz2_regex_chunk_bytes", ctypes.c_uint32, []),
    ("mi355x_bz2_match_lines", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, _vp, ctypes.c_uint8, _vp, _vp,
                                               _vp, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_grep_regex", ctypes.c_int, [_vp, _vp, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_line_hash", ctypes.c_uint64, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64]),
    ("mi355x_bz2_line_hash_chunk_bytes", ctypes.c_uint32, []),
    ("mi355x_bz2_hash_lines", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint64,
                                              _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_reader_line_hashes", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                      ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_take_line_hashes", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int]),
    ("mi355x_bz2_reader_line_hashes_device", ctypes.c_void_p, [_vp]),
    ("mi355x_bz2_reader_distinct_lines", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint64, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_take_distinct_lines", ctypes.c_int, [_vp, _u64p, ctypes.c_uint64]),
    ("mi355x_bz2_field_chunk_bytes", ctypes.c_uint32, []),
    ("mi355x_bz2_field_spans", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8,
                                               ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_field_spans_quoted", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8,
                                                      ctypes.c_uint8, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_reader_field_spans_quoted", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                                                             ctypes.c_uint64, ctypes.c_int, _u64p, ctypes.c_uint8]),
    ("mi355x_bz2_reader_field_columns_quoted", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, _u32p, ctypes.c_uint32,
                                                               ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p, _u64p,
                                                               ctypes.c_uint8]),
    ("mi355x_bz2_gather_fields_tile_bytes", ctypes.c_uint32, []),
    ("mi355x_bz2_gather_fields", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp, _vp, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_field_spans", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                                                      ctypes.c_uint64, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_take_field_spans", ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_int]),
    ("mi355x_bz2_reader_field_columns", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, _u32p, ctypes.c_uint32, ctypes.c_uint64,
                                                        ctypes.c_uint64, ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_field_column", ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_int]),
    ("mi355x_bz2_field_hashes", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8,
                                                ctypes.c_uint32, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_reader_field_hashes", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                                                       ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_take_field_hashes", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int]),
    ("mi355x_bz2_reader_field_groups", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                                                       ctypes.c_uint64, ctypes.c_uint64, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_field_groups", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_parse_field_number", ctypes.c_int64, [ctypes.c_char_p, ctypes.c_uint64]),
    ("mi355x_bz2_field_numbers", ctypes.c_int, [_vp, ctypes.POINTER(ByteSpan), ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint8,
                                                 ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_reader_field_numbers", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64,
                                                        ctypes.c_uint64, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_take_field_numbers", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int]),
    ("mi355x_bz2_reader_field_sums", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint32,
                                                     ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_field_sums", ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_uint64]),
    ("mi355x_bz2_match_fields", ctypes.c_int, [_vp, ctypes.c_char_p, _vp, ctypes.c_uint32, ctypes.c_uint64, _vp, _vp, _vp,
                                                ctypes.c_uint64, ctypes.c_uint64, _vp]),
    ("mi355x_bz2_reader_field_matches", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_char_p, _vp,
                                                        ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64,
                                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_reader_field_in_range", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_int,
                                                         ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64,
                                                         ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_field_matches", ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_int]),
    ("mi355x_bz2_reader_select_lines", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, ctypes.c_char_p, _vp,
                                                       ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                                       ctypes.c_int64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                       ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_match_fields_regex", ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
    ("mi355x_bz2_reader_field_matches_regex", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, _vp, ctypes.c_int,
                                                              ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                                              _u64p, _u64p]),
    ("mi355x_bz2_reader_select_lines_regex", ctypes.c_int, [_vp, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_uint32, _vp, ctypes.c_int,
                                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                                             _u64p, _u64p]),
    ("mi355x_bz2_read_stream_header", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64]),
    ("mi355x_bz2_reader_open_path", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("mi355x_bz2_reader_open_fd", ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(_vp)]),
    ("mi355x_bz2_reader_open_memory", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32,
                                                      ctypes.POINTER(_vp)]),
    ("mi355x_bz2_reader_close", None, [_vp]),
    ("mi355x_bz2_reader_last_error", ctypes.c_char_p, [_vp]),
    ("mi355x_bz2_reader_read", ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_seek", ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_tell", ctypes.c_uint64, [_vp]),
    ("mi355x_bz2_reader_eof", ctypes.c_int, [_vp]),
    ("mi355x_bz2_reader_closed", ctypes.c_int, [_vp]),
    ("mi355x_bz2_reader_size", ctypes.c_int, [_vp, _u64p]),
    ("mi355x_bz2_reader_tell_compressed", ctypes.c_uint64, [_vp]),
    ("mi355x_bz2_reader_block_offsets_complete", ctypes.c_int, [_vp]),
    ("mi355x_bz2_reader_block_offsets", ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_available_block_offsets", ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_set_block_offsets", ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_uint64]),
    ("mi355x_bz2_reader_read_ranges", ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_uint32, _vp, ctypes.c_int, _u64p]),
    ("mi355x_bz2_reader_line_offsets", ctypes.c_int, [_vp, ctypes.c_uint8, _u64p, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_set_line_offsets", ctypes.c_int, [_vp, ctypes.c_uint8, _u64p, _u64p, ctypes.c_uint64]),
    ("mi355x_bz2_reader_line_starts", ctypes.c_int, [_vp, ctypes.c_uint8, _u64p, ctypes.c_uint32, _u64p]),
    ("mi355x_bz2_reader_read_line_ranges", ctypes.c_int, [_vp, ctypes.c_uint8, _u64p, _u64p, ctypes.c_uint32, ctypes.c_int,
                                                           _u64p, _u64p]),
    ("mi355x_bz2_reader_take_line_ranges", ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    ("mi355x_bz2_reader_search", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_take_matches", ctypes.c_int, [_vp, _u64p, ctypes.c_uint64]),
    ("mi355x_bz2_reader_line_numbers", ctypes.c_int, [_vp, ctypes.c_uint8, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_grep", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_uint64,
                                               ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_grep", ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_uint64]),
    ("mi355x_bz2_reader_search_set", ctypes.c_int, [_vp, ctypes.c_char_p, _u32p, ctypes.c_uint32, ctypes.c_uint64,
                                                     ctypes.c_uint64, ctypes.c_uint64, _u64p, _u64p]),
    ("mi355x_bz2_reader_take_set_matches", ctypes.c_int, [_vp, _u64p, _u32p, ctypes.c_uint64]),
    ("mi355x_bz2_reader_grep_set", ctypes.c_int, [_vp, ctypes.c_char_p, _u32p, ctypes.c_uint32, ctypes.c_uint8,
                                                   ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p,
                                                   _u64p]),
    ("mi355x_bz2_reader_search_ex", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                                                    ctypes.c_uint64, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_reader_grep_ex", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint8,
                                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, _u64p,
                                                  _u64p]),
    ("mi355x_bz2_reader_search_set_ex", ctypes.c_int, [_vp, ctypes.c_char_p, _u32p, ctypes.c_uint32, ctypes.c_uint32,
                                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, _u64p, _u64p]),
    ("mi355x_bz2_reader_grep_set_ex", ctypes.c_int, [_vp, ctypes.c_char_p, _u32p, ctypes.c_uint32, ctypes.c_uint32,
                                                      ctypes.c_uint8, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                      ctypes.c_int, _u64p, _u64p]),
    ("mi355x_bz2_reader_join_threads", ctypes.c_int, [_vp]),
    ("mi355x_bz2_reader_set_verify_stream_crc", ctypes.c_int, [_vp, ctypes.c_int]),
    ("mi355x_bz2_reader_streams_verified", ctypes.c_uint64, [_vp]),
    ("mi355x_bz2_reader_statistics", ctypes.c_int, [_vp, ctypes.POINTER(ReaderStats)]),
    ("mi355x_bz2_decompress_buffers", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_void_p), _u64p, ctypes.c_uint32,
                                                      ctypes.c_uint32, ctypes.POINTER(BufferResult), _u64p]),
    ("mi355x_bz2_compress_buffers", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_void_p), _u64p, ctypes.c_uint32,
                                                    ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(CompressResult), _u64p]),
    ("mi355x_bz2_compress_block_map", ctypes.c_int, [_vp, ctypes.c_uint32, _u64p, _u64p, ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_encoder_memory", ctypes.c_int, [_vp, _u64p]),
    ("mi355x_bz2_plan_compress_blocks", ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, _u64p,
                                                        ctypes.c_uint64, _u64p]),
    ("mi355x_bz2_decode_chunk", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint64, ctypes.POINTER(ChunkResult), ctypes.POINTER(BlockResult),
                                               ctypes.c_uint32, ctypes.POINTER(ChunkBoundary), ctypes.c_uint32]),
]

_lib = None


def lib():
    """Load libmi355x_bz2.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first (python -m indexed_bzip2_amd.build). "
                "indexed_bzip2_amd has no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(L, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


def warmup(device: int = 0, background: bool = True):
    """Start the HIP runtime and load the kernels now (0.2 s once per process) instead of inside the first open():
    on a daemon thread by default, so the caller carries on.  Optional; not for processes that fork workers later."""
    L = lib()
    if not background:
        rc = L.mi355x_bz2_warmup(device)
        if rc != 0:
            raise Bz2Error(rc)
        return None
    import threading
    thread = threading.Thread(target=L.mi355x_bz2_warmup, args=(device,), daemon=True)
    thread.start()
    return thread


def status_string(status: int) -> str:
    return lib().mi355x_bz2_status_string(status).decode()


class Bz2Error(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = status_string(status)
        if detail:
            msg += f" ({detail})"
        super().__init__(msg)


def find_magic(data: bytes, magic: int = MAGIC_BLOCK, threads: int = 0):
    L = lib()
    n = L.mi355x_bz2_find_magic(data, len(data), magic, None, 0, threads)
    arr = (ctypes.c_uint64 * max(1, n))()
    L.mi355x_bz2_find_magic(data, len(data), magic, arr, n, threads)
    return list(arr[:n])


def plan_compress_blocks(data, level: int = 9):
    """Input sizes of the blocks libbz2 cuts `data` into at `level` (host only, no GPU)."""
    data = bytes(_byte_view(data))
    n = ctypes.c_uint64()
    rc = lib().mi355x_bz2_plan_compress_blocks(data, len(data), level, None, 0, ctypes.byref(n))
    if rc != OK:
        raise Bz2Error(rc)
    arr = (ctypes.c_uint64 * max(1, n.value))()
    lib().mi355x_bz2_plan_compress_blocks(data, len(data), level, arr, n.value, ctypes.byref(n))
    return list(arr[:n.value])


def _byte_view(obj) -> memoryview:
    """A flat unsigned-byte view of any C-contiguous buffer-protocol object (bytes, bytearray, memoryview, numpy)."""
    view = memoryview(obj)
    if not view.c_contiguous:
        raise ValueError("buffers must be C-contiguous")
    return view.cast("B") if view.format != "B" or view.ndim != 1 else view


SET_MAX_PATTERNS, SET_MAX_PATTERN_BYTES, SET_MAX_BYTES = 1024, 256, 16384


SEARCH_IGNORE_CASE = 1          # MI355X_BZ2_SEARCH_IGNORE_CASE


REGEX_MAX_STATES = 64           # MI355X_BZ2_REGEX_MAX_STATES


class CompiledRegex:
    """A regular expression compiled to the DFA the GPU runs (compile_regex).  .states is the number n of states,
    .transitions a numpy uint8 array [n, 256], .accepts_at_end a numpy uint8 array [n]: state 0 is the start of a line,
    state 1 is "this line has matched" and absorbing, `^` holds in state 0 only and `$` is accepts_at_end."""

    def __init__(self, pattern, ignore_case=False):
        import numpy as np
        if isinstance(pattern, str):
            raise TypeError("the pattern must be a bytes-like object, not str")
        self.pattern = bytes(_byte_view(pattern))
        self.ignore_case = bool(ignore_case)
        self._h = None
        handle = ctypes.c_void_p()
        error = ctypes.create_string_buffer(512)
        rc = lib().mi355x_bz2_regex_compile(self.pattern, len(self.pattern), SEARCH_IGNORE_CASE if ignore_case else 0,
                                            ctypes.byref(handle), error, len(error))
        if rc == ERR_INVALID_ARGUMENT:
            raise ValueError(error.value.decode("latin-1"))
        if rc != OK:
            raise Bz2Error(rc, error.value.decode("latin-1"))
        self._h = handle
        self.states = int(lib().mi355x_bz2_regex_states(handle))
        self.transitions = np.empty((self.states, 256), dtype=np.uint8)
        self.accepts_at_end = np.empty(self.states, dtype=np.uint8)
        lib().mi355x_bz2_regex_table(handle, self.transitions.ctypes.data, self.accepts_at_end.ctypes.data)
        self.transitions.setflags(write=False)
        self.accepts_at_end.setflags(write=False)

    def __del__(self):
        if getattr(self, "_h", None) is not None and _lib is not None:
            _lib.mi355x_bz2_regex_free(self._h)
            self._h = None

    def __repr__(self):
        return f"CompiledRegex({self.pattern!r}, ignore_case={self.ignore_case}, states={self.states})"


def compile_regex(pattern, ignore_case=False):
    """Compile `pattern` (bytes-like; a subset of Python's bytes `re` syntax, every accepted pattern with Python's meaning
    under re.DOTALL) for grep_regex and Decoder.match_lines.  Needs no GPU.  A pattern outside the subset, or one whose
    DFA needs more than 64 states, is a ValueError that names the construct and its offset."""
    return CompiledRegex(pattern, ignore_case)


def regex_chunk_bytes():
    """The bytes of a span that one GPU lane walks in match_lines (mi355x_bz2_regex_chunk_bytes)."""
    return int(lib().mi355x_bz2_regex_chunk_bytes())


class LineHashSummary(ctypes.Structure):
    """mi355x_bz2_line_hash_summary"""
    _fields_ = [("head_hash", ctypes.c_uint64), ("head_xl", ctypes.c_uint64), ("tail_hash", ctypes.c_uint64),
                ("tail_xl", ctypes.c_uint64), ("count", ctypes.c_uint64), ("has_delimiter", ctypes.c_uint32),
                ("tail_non_empty", ctypes.c_uint32)]


def line_hash(content, seed=0):
    """The hash line_hashes gives a line with this content (bytes-like, without the delimiter), on the CPU: p = 2^61 - 1,
    x = 256 + splitmix64(seed) % (p - 256), h = 0 and h = (h * x + b + 1) % p for every byte b.  Needs no GPU."""
    if isinstance(content, str):
        raise TypeError("the content must be a bytes-like object, not str")
    seed = int(seed)
    if seed < 0 or seed >= 2**64:
        raise ValueError("seed must not be negative and must fit 64 bits")
    data = bytes(_byte_view(content))
    return int(lib().mi355x_bz2_line_hash(data, len(data), seed))


def line_hash_chunk_bytes():
    """The bytes of a span that one GPU lane walks in hash_lines (mi355x_bz2_line_hash_chunk_bytes)."""
    return int(lib().mi355x_bz2_line_hash_chunk_bytes())


class FieldSummary(ctypes.Structure):
    """mi355x_bz2_field_summary"""
    _fields_ = [("count", ctypes.c_uint64), ("first_nl", ctypes.c_uint64), ("tail_start", ctypes.c_uint64),
                ("tail_field_start", ctypes.c_uint64), ("tail_field_end", ctypes.c_uint64), ("head_delims", ctypes.c_uint32),
                ("tail_delims", ctypes.c_uint32), ("has_delimiter", ctypes.c_uint32), ("tail_non_empty", ctypes.c_uint32)]


class QuotedFieldSummary(ctypes.Structure):
    """mi355x_bz2_quoted_field_summary"""
    _fields_ = [("count", ctypes.c_uint64), ("first_nl", ctypes.c_uint64), ("tail_start", ctypes.c_uint64),
                ("tail_field_start", ctypes.c_uint64), ("tail_field_end", ctypes.c_uint64), ("head_delims", ctypes.c_uint32 * 2),
                ("tail_delims", ctypes.c_uint32), ("has_delimiter", ctypes.c_uint32), ("tail_non_empty", ctypes.c_uint32),
                ("head_quote_parity", ctypes.c_uint32), ("tail_in_quote", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def field_chunk_bytes():
    """The bytes of a span that one GPU lane walks in field_spans (mi355x_bz2_field_chunk_bytes)."""
    return int(lib().mi355x_bz2_field_chunk_bytes())


def gather_fields_tile_bytes():
    """The bytes of the destination that one GPU workgroup writes in gather_fields (mi355x_bz2_gather_fields_tile_bytes)."""
    return int(lib().mi355x_bz2_gather_fields_tile_bytes())


FIELD_MISSING = 2**61 - 1      # MI355X_BZ2_FIELD_MISSING: the key of a line that has no such field


class FieldHashSummary(ctypes.Structure):
    """mi355x_bz2_field_hash_summary"""
    _fields_ = [("count", ctypes.c_uint64), ("first_nl", ctypes.c_uint64), ("tail_start", ctypes.c_uint64),
                ("tail_field_start", ctypes.c_uint64), ("tail_field_end", ctypes.c_uint64), ("head_hash", ctypes.c_uint64),
                ("head_xl", ctypes.c_uint64), ("tail_hash", ctypes.c_uint64), ("tail_xl", ctypes.c_uint64),
                ("tail_start_hash", ctypes.c_uint64), ("tail_end_hash", ctypes.c_uint64), ("head_delims", ctypes.c_uint32),
                ("tail_delims", ctypes.c_uint32), ("has_delimiter", ctypes.c_uint32), ("tail_non_empty", ctypes.c_uint32)]


FIELD_NOT_A_NUMBER = -2**63          # MI355X_BZ2_FIELD_NOT_A_NUMBER: the field is present and is no number
FIELD_NUMBER_MISSING = -2**63 + 1    # MI355X_BZ2_FIELD_NUMBER_MISSING: the line has no such field


class FieldText(ctypes.Structure):
    """mi355x_bz2_field_text: the first 19 bytes of a byte string and its size, saturated at 20"""
    _fields_ = [("size", ctypes.c_uint8), ("bytes", ctypes.c_uint8 * 19)]

    def as_tuple(self):
        """(size, the bytes that are kept)"""
        return int(self.size), bytes(self.bytes[:min(self.size, 19)])


def parse_field_number(content):
    """The number field_ints gives a field with these bytes, on the CPU: int(content) if the bytes match
    [+-]?[0-9]{1,18} from end to end, else None.  No whitespace, no '_', no hex, no floats; leading zeros count towards
    the 18 digits; b"-0" is 0; b"", b"+", b"-" and 19 or more digits are no numbers.  This is not awk's strtod and not
    Python's int(), which accept more.  Needs no GPU."""
    if isinstance(content, str):
        raise TypeError("the content must be a bytes-like object, not str")
    data = bytes(_byte_view(content))
    value = int(lib().mi355x_bz2_parse_field_number(data, len(data)))
    return None if value == FIELD_NOT_A_NUMBER else value


def pattern_set(patterns, check=True):
    """A set of patterns for the *_set calls: (the patterns concatenated, their sizes as a uint32 array, their number).
    `patterns` is any sequence of bytes-like objects; a str element, or a bare bytes-like object in place of the sequence,
    is a TypeError.  With `check`, a set outside the limits of the search -- 1 to 1 024 patterns of 1 to 256 bytes, at
    most 16 384 bytes in total -- is a ValueError (without it, the native call refuses the set)."""
    if isinstance(patterns, (str, bytes, bytearray, memoryview)):
        raise TypeError("patterns must be a sequence of bytes-like objects, not one " + type(patterns).__name__)
    items = []
    for pattern in patterns:
        if isinstance(pattern, str):
            raise TypeError("a pattern must be bytes-like, not str")
        items.append(bytes(memoryview(pattern)))      # TypeError for what is not bytes-like
    if check:
        if not 1 <= len(items) <= SET_MAX_PATTERNS:
            raise ValueError(f"the set must have 1 to {SET_MAX_PATTERNS} patterns, not {len(items)}")
        for i, pattern in enumerate(items):
            if not 1 <= len(pattern) <= SET_MAX_PATTERN_BYTES:
                raise ValueError(f"every pattern must have 1 to {SET_MAX_PATTERN_BYTES} bytes, pattern {i} has {len(pattern)}")
        if sum(map(len, items)) > SET_MAX_BYTES:
            raise ValueError(f"the patterns must have at most {SET_MAX_BYTES} bytes in total, not {sum(map(len, items))}")
    sizes = (ctypes.c_uint32 * max(1, len(items)))(*[len(pattern) for pattern in items])
    return b"".join(items), sizes, len(items)


FIELD_VALUES_MAX = 1024          # of a where_field predicate: values, bytes per value, bytes in total
FIELD_VALUE_BYTES_MAX = 256
FIELD_VALUES_BYTES_MAX = 16384
FIELD_NUMBER_MAX = 10**18 - 1    # the largest number a field can be; the least is its negative


def value_set(values, check=True):
    """The values of a where_field predicate: (the values concatenated, their sizes as a uint32 array, their number).
    `values` is any sequence of bytes-like objects; a str element, or a bare bytes-like object in place of the sequence,
    is a TypeError.  With `check`, a set outside the limits -- 1 to 1 024 values of 0 to 256 bytes, at most 16 384 bytes
    in total -- is a ValueError (without it, the native call refuses the set).  The empty value is allowed."""
    if isinstance(values, (str, bytes, bytearray, memoryview)):
        raise TypeError("values must be a sequence of bytes-like objects, not one " + type(values).__name__)
    items = []
    for value in values:
        if isinstance(value, str):
            raise TypeError("a value must be bytes-like, not str")
        items.append(bytes(memoryview(value)))      # TypeError for what is not bytes-like
    if check:
        if not 1 <= len(items) <= FIELD_VALUES_MAX:
            raise ValueError(f"the set must have 1 to {FIELD_VALUES_MAX} values, not {len(items)}")
        for i, value in enumerate(items):
            if len(value) > FIELD_VALUE_BYTES_MAX:
                raise ValueError(f"value {i} has {len(value)} bytes, more than {FIELD_VALUE_BYTES_MAX}")
        if sum(map(len, items)) > FIELD_VALUES_BYTES_MAX:
            raise ValueError(f"the values must have at most {FIELD_VALUES_BYTES_MAX} bytes in total, not {sum(map(len, items))}")
    sizes = (ctypes.c_uint32 * max(1, len(items)))(*[len(value) for value in items])
    return b"".join(items), sizes, len(items)


def number_range(between):
    """The bounds of a where_field range as the native calls take them: (has_lo, lo, has_hi, hi).  `between` is (lo, hi),
    each a Python int or None for an open side; a bound is clipped to [-(10**18 - 1), 10**18 - 1], the numbers a field
    can be."""
    try:
        lo, hi = between
    except (TypeError, ValueError):
        raise ValueError("between must be a pair (lo, hi), each an int or None") from None
    out = []
    for bound in (lo, hi):
        if bound is None:
            out += [0, 0]
            continue
        if isinstance(bound, bool) or not isinstance(bound, int):
            raise TypeError("a bound must be an int or None, not " + type(bound).__name__)
        out += [1, max(-FIELD_NUMBER_MAX, min(FIELD_NUMBER_MAX, bound))]
    return tuple(out)


class _KeptInputs(tuple):
    """(previous, current) host buffers of set_input_host_async."""


def _with_device_copies(what, hosts, call):
    """call(*pointers) with one device array per numpy array of `hosts`, all in one device allocation: filled from the host
    arrays before the call, copied back to them behind it, and freed whatever happens."""
    # device memory from the HIP runtime the library itself is linked to (it is loaded already)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    total = sum(host.nbytes for host in hosts)
    device = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(device), total) != 0:
        raise Bz2Error(101, f"{what}: no device memory for {total} bytes")
    try:
        pointers = [ctypes.c_void_p(device.value + sum(host.nbytes for host in hosts[:k])) for k in range(len(hosts))]
        for host, pointer in zip(hosts, pointers):
            if hip.hipMemcpy(pointer, host.ctypes.data, host.nbytes, 1) != 0:           # hipMemcpyHostToDevice
                raise Bz2Error(101, f"{what}: the copy to the device failed")
        call(*pointers)
        for host, pointer in zip(hosts, pointers):
            if hip.hipMemcpy(host.ctypes.data, pointer, host.nbytes, 2) != 0:           # hipMemcpyDeviceToHost
                raise Bz2Error(101, f"{what}: the copy from the device failed")
    finally:
        hip.hipFree(device)


def _field_query_arguments(newline, delimiter, field):
    """(newline byte, delimiter byte, field) of a field query on the last batch's output, checked."""
    nl, dl = bytes(newline), bytes(delimiter)
    if len(nl) != 1 or len(dl) != 1:
        raise ValueError("newline and delimiter must be exactly one byte each")
    field = int(field)
    if field < 0 or field > 1023:
        raise ValueError("field must be between 0 and 1023")
    if nl == dl:
        raise ValueError("delimiter and newline must differ")
    return nl[0], dl[0], field


def _field_summary_dict(s, heads):
    """The field members of a span's summary (FieldSummary, or FieldHashSummary, which repeats them); `heads` starts at the
    span's head positions.  None for a position the span does not reach."""
    none = 2**64 - 1
    return {"count": int(s.count), "has_delimiter": bool(s.has_delimiter),
            "first_nl": None if s.first_nl == none else int(s.first_nl),
            "head_positions": [int(v) for v in heads[:s.head_delims]],
            "tail_start": int(s.tail_start), "tail_delims": int(s.tail_delims),
            "tail_field_start": None if s.tail_field_start == none else int(s.tail_field_start),
            "tail_field_end": None if s.tail_field_end == none else int(s.tail_field_end),
            "tail_non_empty": bool(s.tail_non_empty)}


def _quoted_field_summary_dict(s, heads, cap):
    """_field_summary_dict for a QuotedFieldSummary; `heads` starts at the span's two lists of `cap` head positions."""
    none = 2**64 - 1
    return {"count": int(s.count), "has_delimiter": bool(s.has_delimiter),
            "first_nl": None if s.first_nl == none else int(s.first_nl),
            "head_positions": [[int(v) for v in heads[h * cap:h * cap + s.head_delims[h]]] for h in (0, 1)],
            "head_quote_parity": bool(s.head_quote_parity),
            "tail_start": int(s.tail_start), "tail_delims": int(s.tail_delims),
            "tail_field_start": None if s.tail_field_start == none else int(s.tail_field_start),
            "tail_field_end": None if s.tail_field_end == none else int(s.tail_field_end),
            "tail_in_quote": bool(s.tail_in_quote), "tail_non_empty": bool(s.tail_non_empty)}


class Decoder:
    """One decoder context = one GPU + one HIP stream (mi355x_bz2_ctx)."""

    KEEP_STAGES = 1

    def __init__(self, device: int = -1, max_batch_blocks: int = 0, flags: int = 0):
        self._h = _vp()
        cfg = Config(device, max_batch_blocks, flags, 0)
        rc = lib().mi355x_bz2_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != OK:
            raise Bz2Error(rc)
        self._input_ref = None
        self.last_results = []

    def close(self):
        if self._h:
            lib().mi355x_bz2_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            raise Bz2Error(rc, lib().mi355x_bz2_last_error(self._h).decode())

    def set_input(self, data: bytes):
        self._check(lib().mi355x_bz2_set_input_host(self._h, data, len(data)))

    def set_input_host_async(self, ptr: int, size: int, keepalive=None):
        """Queue the H2D copy of `size` bytes at host address `ptr` (page-locked memory) on the decoder's input stream
        and return: the next begin_batch / decode_batch is ordered behind it.  May be called while a batch is in flight
        (the bytes of the next one).  The memory must stay valid until the batch that uses it has ended."""
        # the previous input may still be on its way to the GPU or in use by the batch in flight: keep it too, and no more
        # (the context has two input buffers: the batch in flight's and the next one's)
        previous = self._input_ref
        self._input_ref = (previous[1] if isinstance(previous, _KeptInputs) else previous, keepalive)
        self._input_ref = _KeptInputs(self._input_ref)
        self._check(lib().mi355x_bz2_set_input_host_async(self._h, ptr, size))

    def set_input_device(self, ptr: int, size: int, keepalive=None):
        self._input_ref = keepalive
        self._check(lib().mi355x_bz2_set_input_device(self._h, ptr, size))

    def share_input(self, other: "Decoder"):
        """Decode from the bytes `other` made resident (no copy); `other` is kept alive."""
        self._input_ref = other
        self._check(lib().mi355x_bz2_share_input(self._h, other._h))

    def decode_batch(self, offsets):
        n = len(offsets)
        offs = (ctypes.c_uint64 * max(1, n))(*offsets)
        res = (BlockResult * max(1, n))()
        total = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_decode_batch(self._h, offs, n, res, ctypes.byref(total)))
        self.last_results = [res[i].as_dict() for i in range(n)]
        return self.last_results, total.value

    @staticmethod
    def make_arrays(offsets):
        """ctypes arrays for decode_batch_into: (offsets, results), reusable across calls."""
        n = len(offsets)
        return (ctypes.c_uint64 * max(1, n))(*offsets), (BlockResult * max(1, n))()

    def decode_batch_into(self, offsets_array, n: int, results_array) -> int:
        """decode_batch without building Python dicts (2 560 blocks x 12 fields cost milliseconds): the results stay in
        `results_array` (ctypes BlockResult[n], e.g. viewed through numpy.frombuffer).  Returns the decoded size."""
        total = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_decode_batch(self._h, offsets_array, n, results_array, ctypes.byref(total)))
        self.last_results = None
        return total.value

    def begin_batch(self, offsets_array, n: int):
        """First half of decode_batch_into: queues the batch up to its decoded sizes and returns at once."""
        self._check(lib().mi355x_bz2_decode_batch_begin(self._h, offsets_array, n))

    def end_batch(self, results_array) -> int:
        """Second half: output offsets, RLE expansion, CRC; returns the decoded size."""
        total = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_decode_batch_end(self._h, results_array, ctypes.byref(total)))
        self.last_results = None
        return total.value

    def decode_chunk(self, data: bytes, chunk_offset: int, until_offset: int, max_decoded: int = 2**63):
        """rapidgzip Bzip2Chunk::decodeChunk counterpart (mi355x_bz2_decode_chunk): `data` = the bytes given to
        set_input().  Returns (chunk dict, block dicts, footers [(encoded bits, decoded offset)], chunk bytes)."""
        cap = 4096
        res = ChunkResult()
        blocks = (BlockResult * cap)()
        footers = (ChunkBoundary * cap)()
        self._check(lib().mi355x_bz2_decode_chunk(self._h, data, len(data), chunk_offset, until_offset, max_decoded,
                                                  ctypes.byref(res), blocks, cap, footers, cap))
        d = res.as_dict()
        payload = self.copy_output(d["data_offset"], d["decoded_size"]) if d["status"] == OK and d["decoded_size"] else b""
        return (d, [blocks[i].as_dict() for i in range(min(cap, d["n_blocks"]))],
                [(footers[i].encoded_offset_bits, footers[i].decoded_offset) for i in range(min(cap, d["n_footers"]))],
                payload)

    def decompress_buffers(self, buffers, max_launch_blocks: int = 0):
        """mi355x_bz2_decompress_buffers over C-contiguous byte buffers: returns (list of BufferResult dicts, total).
        The bytes are then [output_offset, output_offset + decoded_size) of the output: copy_output, gather_output,
        output_device_ptr (copy_output_begin refuses it).  Replaces the decoder's input (set_input)."""
        import numpy as np
        arrays = [np.frombuffer(_byte_view(b), dtype=np.uint8) for b in buffers]   # no copy, read-only is fine
        n = len(arrays)
        ptrs = (ctypes.c_void_p * max(1, n))(*[a.ctypes.data if a.size else None for a in arrays])
        sizes = (ctypes.c_uint64 * max(1, n))(*[a.size for a in arrays])
        res = (BufferResult * max(1, n))()
        total = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_decompress_buffers(self._h, ptrs, sizes, n, max_launch_blocks, res,
                                                        ctypes.byref(total)))
        return [res[i].as_dict() for i in range(n)], total.value

    def compress_buffers(self, buffers, level: int = 9, max_launch_blocks: int = 0):
        """mi355x_bz2_compress_buffers over C-contiguous byte buffers: returns (list of CompressResult dicts, total).
        Buffer i's stream is [output_offset, output_offset + compressed_size) of the output (copy_output,
        gather_output, output_device_ptr)."""
        import numpy as np
        arrays = [np.frombuffer(_byte_view(b), dtype=np.uint8) for b in buffers]
        n = len(arrays)
        ptrs = (ctypes.c_void_p * max(1, n))(*[a.ctypes.data if a.size else None for a in arrays])
        sizes = (ctypes.c_uint64 * max(1, n))(*[a.size for a in arrays])
        res = (CompressResult * max(1, n))()
        total = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_compress_buffers(self._h, ptrs, sizes, n, level, max_launch_blocks, res,
                                                      ctypes.byref(total)))
        return [res[i].as_dict() for i in range(n)], total.value

    def compress_block_map(self, buffer: int) -> dict:
        """Block map {bit offset: decoded offset} of buffer `buffer` of the last compress_buffers call."""
        n = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_compress_block_map(self._h, buffer, None, None, 0, ctypes.byref(n)))
        bits = (ctypes.c_uint64 * max(1, n.value))()
        byts = (ctypes.c_uint64 * max(1, n.value))()
        self._check(lib().mi355x_bz2_compress_block_map(self._h, buffer, bits, byts, n.value, ctypes.byref(n)))
        return {bits[i]: byts[i] for i in range(n.value)}

    def encoder_memory(self) -> int:
        """bytes of HBM the encoder's scratch holds (0 before the first compress call)"""
        b = ctypes.c_uint64(0)
        self._check(lib().mi355x_bz2_encoder_memory(self._h, ctypes.byref(b)))
        return b.value

    def find_magic(self, magic: int = MAGIC_BLOCK):
        """Magic-bit scan of the resident input on the GPU (k_find_magic)."""
        n = ctypes.c_uint64()
        self._check(lib().mi355x_bz2_find_magic_device(self._h, magic, None, 0, ctypes.byref(n)))
        arr = (ctypes.c_uint64 * max(1, n.value))()
        self._check(lib().mi355x_bz2_find_magic_device(self._h, magic, arr, n.value, ctypes.byref(n)))
        return list(arr[:n.value])

    def crc32_device(self, device_ptr: int, sizes):
        """bzip2 CRC-32 of consecutive pieces (`sizes` bytes each) of a 16-byte aligned device buffer."""
        n = len(sizes)
        arr = (ctypes.c_uint64 * max(1, n))(*sizes)
        out = (ctypes.c_uint32 * max(1, n))()
        self._check(lib().mi355x_bz2_crc32_device(self._h, ctypes.c_void_p(device_ptr), arr, n, out))
        return list(out[:n])

    @staticmethod
    def _pieces(pieces):
        pieces = [(int(s), int(d), int(n)) for s, d, n in pieces]
        arr = (GatherPiece * max(1, len(pieces)))(*[GatherPiece(s, d, n) for s, d, n in pieces])
        return pieces, arr

    def gather_output(self, pieces) -> bytes:
        """k_gather on the host path: `pieces` = [(src_offset, dst_offset, size)] of the last batch's output; returns the
        destination, max(dst_offset + size) bytes long (bytes no piece covers are zero)."""
        pieces, arr = self._pieces(pieces)
        total = max((d + n for _, d, n in pieces), default=0)
        buf = ctypes.create_string_buffer(max(1, total))
        self._check(lib().mi355x_bz2_gather_output(self._h, arr, len(pieces), buf, 0))
        return buf.raw[:total]

    def gather_output_to_device(self, pieces, device_ptr: int):
        """The same into device memory at `device_ptr` (on the decoder's device): each piece written in place."""
        pieces, arr = self._pieces(pieces)
        self._check(lib().mi355x_bz2_gather_output(self._h, arr, len(pieces), ctypes.c_void_p(device_ptr), 1))

    def count_byte(self, value: int, spans):
        """k_count_byte: how often the byte `value` occurs in each span [(offset, size)] of the last batch's output."""
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        out = (ctypes.c_uint64 * max(1, len(spans)))()
        self._check(lib().mi355x_bz2_count_byte(self._h, arr, len(spans), value, out))
        return list(out[:len(spans)])

    def find_byte(self, value: int, queries):
        """k_find_byte: for each query (offset, size, rank) the offset in the last batch's output of the rank-th
        (1-based) byte `value` in the span, or None if the span holds fewer."""
        queries = [(int(o), int(n), int(r)) for o, n, r in queries]
        arr = (ByteQuery * max(1, len(queries)))(*[ByteQuery(o, n, r) for o, n, r in queries])
        out = (ctypes.c_uint64 * max(1, len(queries)))()
        self._check(lib().mi355x_bz2_find_byte(self._h, arr, len(queries), value, out))
        return [None if p == 2**64 - 1 else p for p in out[:len(queries)]]

    def rank_byte(self, queries, value: int):
        """k_rank_byte: for each query (offset, size, position) the number of bytes equal to `value` in
        [offset, position) of the last batch's output; offset <= position <= offset + size."""
        arr = (RankQuery * max(1, len(queries)))(*[RankQuery(o, n, p) for o, n, p in queries])
        out = (ctypes.c_uint64 * max(1, len(queries)))()
        self._check(lib().mi355x_bz2_rank_byte(self._h, arr, len(queries), value, out))
        return [out[i] for i in range(len(queries))]

    def count_bytes(self, pattern, spans, *, ignore_case=False):
        """k_count_bytes: how often the byte string `pattern` (1 to 256 bytes) occurs in each span [(offset, size)] of the
        last batch's output.  A match lies inside its span; matches that overlap themselves all count.  ignore_case=True:
        the folding instantiation, which compares pattern and data under bytes.lower()."""
        flags = SEARCH_IGNORE_CASE if ignore_case else 0
        pattern = bytes(pattern)
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        out = (ctypes.c_uint64 * max(1, len(spans)))()
        self._check(lib().mi355x_bz2_count_bytes_ex(self._h, arr, len(spans), pattern, len(pattern), flags, out))
        return list(out[:len(spans)])

    def find_bytes(self, pattern, spans, capacity=None, *, ignore_case=False):
        """k_count_bytes, k_scan_tiles, k_emit_bytes: (positions, counts) -- the offsets in the last batch's output at
        which `pattern` occurs, span by span and ascending within a span, the first `capacity` of them (None: all), and
        the true count of every span."""
        flags = SEARCH_IGNORE_CASE if ignore_case else 0
        pattern = bytes(pattern)
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        counts = (ctypes.c_uint64 * max(1, len(spans)))()
        if capacity is None:
            self._check(lib().mi355x_bz2_count_bytes_ex(self._h, arr, len(spans), pattern, len(pattern), flags, counts))
            capacity = sum(counts[:len(spans)])
        positions = (ctypes.c_uint64 * max(1, capacity))()
        self._check(lib().mi355x_bz2_find_bytes_ex(self._h, arr, len(spans), pattern, len(pattern), flags, positions, capacity,
                                                   counts))
        found = min(capacity, sum(counts[:len(spans)]))
        return list(positions[:found]), list(counts[:len(spans)])

    def count_bytes_set(self, patterns, spans, *, ignore_case=False):
        """k_count_set: (counts, per_pattern) -- the number of (position, pattern) pairs in each span [(offset, size)] of
        the last batch's output, and how often each pattern of the set occurs over all spans."""
        flags = SEARCH_IGNORE_CASE if ignore_case else 0
        data, sizes, k = pattern_set(patterns, check=False)
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        counts = (ctypes.c_uint64 * max(1, len(spans)))()
        each = (ctypes.c_uint64 * max(1, k))()
        self._check(lib().mi355x_bz2_count_bytes_set_ex(self._h, arr, len(spans), data, sizes, k, flags, counts, each))
        return list(counts[:len(spans)]), list(each[:k])

    def find_bytes_set(self, patterns, spans, capacity=None, *, ignore_case=False):
        """k_count_set, k_scan_tiles, k_emit_set: (positions, ids, counts) -- the pairs (offset in the last batch's output,
        index of the pattern in the set), span by span and by ascending (position, id) within a span, the first `capacity`
        of them (None: all), and the true number of pairs of every span."""
        flags = SEARCH_IGNORE_CASE if ignore_case else 0
        data, sizes, k = pattern_set(patterns, check=False)
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        counts = (ctypes.c_uint64 * max(1, len(spans)))()
        if capacity is None:
            self._check(lib().mi355x_bz2_count_bytes_set_ex(self._h, arr, len(spans), data, sizes, k, flags, counts, None))
            capacity = sum(counts[:len(spans)])
        positions = (ctypes.c_uint64 * max(1, capacity))()
        ids = (ctypes.c_uint32 * max(1, capacity))()
        self._check(lib().mi355x_bz2_find_bytes_set_ex(self._h, arr, len(spans), data, sizes, k, flags, positions, ids, capacity,
                                                       counts, None))
        found = min(capacity, sum(counts[:len(spans)]))
        return list(positions[:found]), list(ids[:found]), list(counts[:len(spans)])

    def match_lines(self, spans, regex, newline=b"\n", capacity=None):
        """k_regex_chunks, k_regex_link, k_scan_tiles, k_regex_emit: the summary of every span [(offset, size)] of the last
        batch's output under `regex` (compile_regex, or a pattern to compile), read as a stretch of lines that a line may
        enter and leave -> (head_maps, has_delimiter, exit_states, positions, counts): head_maps a numpy uint8 array
        [spans, 64] (the state behind the span's first line for every entry state), has_delimiter and exit_states one
        value per span, positions one offset inside every line that starts in its span and matches there, span by span
        and ascending, the first `capacity` of them (None: all; 0: no emitting pass), counts their true number per span."""
        import numpy as np
        if not isinstance(regex, CompiledRegex):
            regex = compile_regex(regex)
        nl = bytes(newline)
        if len(nl) != 1:
            raise ValueError("newline must be exactly one byte")
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        head_maps = np.zeros((len(spans), REGEX_MAX_STATES), dtype=np.uint8)
        has_delimiter = np.zeros(max(1, len(spans)), dtype=np.uint8)
        exit_states = np.zeros(max(1, len(spans)), dtype=np.uint8)
        counts = (ctypes.c_uint64 * max(1, len(spans)))()

        def call(positions, room):
            self._check(lib().mi355x_bz2_match_lines(self._h, arr, len(spans), regex._h, nl[0],
                                                     head_maps.ctypes.data if len(spans) else None,
                                                     has_delimiter.ctypes.data, exit_states.ctypes.data, positions, room, counts))
        if capacity is None:
            call(None, 0)
            capacity = sum(counts[:len(spans)])
        positions = (ctypes.c_uint64 * max(1, capacity))()
        call(positions, capacity)
        found = min(capacity, sum(counts[:len(spans)]))
        return (head_maps, [bool(v) for v in has_delimiter[:len(spans)]], [int(v) for v in exit_states[:len(spans)]],
                list(positions[:found]), list(counts[:len(spans)]))

    def hash_lines(self, spans, newline=b"\n", seed=0, capacity=None, room=None):
        """k_linehash_chunks, k_linehash_link, k_scan_tiles, k_linehash_emit: the summary of every span [(offset, size)] of
        the last batch's output, read as a stretch of lines that a line may enter and leave, and the hashes of the lines
        the spans close -> (summaries, hashes): one dict per span (head and tail as (h, xl), has_delimiter,
        tail_non_empty, count) and a numpy uint64 array of `room` values (default: capacity) that were all ones before the
        call and of which the call may write the first `capacity` (None: as many as there are closed lines)."""
        import numpy as np
        nl = bytes(newline)
        if len(nl) != 1:
            raise ValueError("newline must be exactly one byte")
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        summaries = (LineHashSummary * max(1, len(spans)))()

        def call(device, capacity):
            self._check(lib().mi355x_bz2_hash_lines(self._h, arr, len(spans), nl[0], int(seed), summaries, device, capacity))
        if capacity is None:
            call(None, 0)
            capacity = sum(s.count for s in summaries[:len(spans)])
        room = capacity if room is None else max(int(room), capacity)
        hashes = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        _with_device_copies("hash_lines", [hashes], lambda device: call(device, capacity))
        out = [{"head": (s.head_hash, s.head_xl), "tail": (s.tail_hash, s.tail_xl), "has_delimiter": bool(s.has_delimiter),
                "tail_non_empty": bool(s.tail_non_empty), "count": int(s.count)} for s in summaries[:len(spans)]]
        return out, hashes[:room]

    def field_spans(self, spans, field, delimiter=b"\t", newline=b"\n", capacity=None, room=None, *, quote=None):
        """k_field_chunks, k_field_link, k_scan_tiles, k_field_emit, k_field_sizes: the summary for field `field` of every
        span [(offset, size)] of the last batch's output, read as a stretch of lines that a line may enter and leave, and
        where the field lies in the lines the spans close -> (summaries, starts, sizes): one dict per span (count,
        has_delimiter, first_nl, head_positions, tail_start, tail_delims, tail_field_start, tail_field_end,
        tail_non_empty; None for a position the span does not reach) and two numpy arrays, uint64 and int64, of `room`
        values (default: capacity) that were all ones before the call and of which the call may write the first
        `capacity` (None: as many as there are closed lines).  A start is an offset in the output.

        With quote (one byte, not the delimiter or the newline) mi355x_bz2_field_spans_quoted: k_field_chunks_quoted,
        k_field_link_quoted, k_scan_tiles, k_field_emit_quoted, k_field_sizes, k_field_unquote.  starts and sizes are the
        fields' contents; a summary is raw and has head_positions as a pair of lists, the span entered outside and inside
        quotes, and head_quote_parity and tail_in_quote besides."""
        import numpy as np
        nl, dl, field = _field_query_arguments(newline, delimiter, field)
        if quote is not None:
            if not isinstance(quote, (bytes, bytearray, memoryview)):
                raise ValueError("quote must be exactly one byte that differs from delimiter and newline")
            quote = bytes(quote)
            if len(quote) != 1 or quote[0] in (nl, dl):
                raise ValueError("quote must be exactly one byte that differs from delimiter and newline")
        lists = 1 if quote is None else 2
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        summaries = ((FieldSummary if quote is None else QuotedFieldSummary) * max(1, len(spans)))()
        heads = np.zeros(max(1, len(spans) * lists * (field + 1)), dtype=np.uint64)

        def call(starts, sizes, capacity):
            if quote is None:
                self._check(lib().mi355x_bz2_field_spans(self._h, arr, len(spans), nl, dl, field, summaries, heads.ctypes.data,
                                                         starts, sizes, capacity))
            else:
                self._check(lib().mi355x_bz2_field_spans_quoted(self._h, arr, len(spans), nl, dl, quote[0], field, summaries,
                                                                heads.ctypes.data, starts, sizes, capacity))
        if capacity is None:
            call(None, None, 0)
            capacity = sum(s.count for s in summaries[:len(spans)])
        room = capacity if room is None else max(int(room), capacity)
        starts = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        sizes = np.full(max(1, room), -1 - 2**62, dtype=np.int64)
        _with_device_copies("field_spans", [starts, sizes], lambda *device: call(*device, capacity))
        if quote is None:
            out = [_field_summary_dict(s, heads[i * (field + 1):]) for i, s in enumerate(summaries[:len(spans)])]
        else:
            out = [_quoted_field_summary_dict(s, heads[2 * i * (field + 1):], field + 1) for i, s in enumerate(summaries[:len(spans)])]
        return out, starts[:room], sizes[:room]

    def gather_fields(self, starts, sizes, base=0, room=None, capacity=None, dst=True, fill=0xA5, misalign=0):
        """k_fieldcol_sums, k_fieldcol_top, k_fieldcol_offsets, k_field_gather: the spans (starts[i] - base, sizes[i]) of
        the last batch's output -- field_spans' two arrays -- packed back to back -> (total, offsets, data): the sum of
        max(size, 0), a numpy uint64 array of their n + 1 exclusive prefix sums, and a numpy uint8 array of `room` bytes
        (default: the total the sizes give) that all were `fill` before the call and of which the call writes the first
        `total` if total <= capacity (default: room).  dst=False: no destination (data is None).  The destination begins
        `misalign` bytes (0 to 15) behind a 16-byte boundary.  A refused call raises Bz2Error, which carries the
        destination as the call left it in `.destination`."""
        import numpy as np
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        if starts.ndim != 1 or starts.shape != sizes.shape:
            raise ValueError("starts and sizes must be one-dimensional and equally long")
        if not 0 <= int(misalign) <= 15:
            raise ValueError("misalign must be between 0 and 15")
        n = int(starts.size)
        if room is None:
            room = int(np.maximum(sizes, 0).sum())
        capacity = int(room) if capacity is None else int(capacity)
        if capacity > room:
            raise ValueError("the capacity must not exceed the room")
        offsets = np.full(n + 1, 2**64 - 1, dtype=np.uint64)
        hosts = [np.resize(starts, max(1, n)), np.resize(sizes, max(1, n)), offsets]
        # the device arrays lie back to back from an aligned allocation: pad so that the destination begins as asked
        before = sum(host.nbytes for host in hosts)
        hosts.append(np.zeros((-before) % 16 + int(misalign), dtype=np.uint8))
        data = np.full(max(1, int(room)), fill, dtype=np.uint8)
        hosts.append(data)
        total = ctypes.c_uint64(2**64 - 1)
        status = []

        def call(d_starts, d_sizes, d_offsets, _, d_data):
            status.append(lib().mi355x_bz2_gather_fields(self._h, d_starts, d_sizes, n, int(base), d_offsets,
                                                         d_data if dst else None, capacity, ctypes.byref(total)))
        _with_device_copies("gather_fields", hosts, call)
        if status[0] != OK:
            error = Bz2Error(status[0], lib().mi355x_bz2_last_error(self._h).decode())
            error.destination = data[:int(room)]
            raise error
        return total.value, offsets, (data[:int(room)] if dst else None)

    def field_hashes(self, spans, field, delimiter=b"\t", newline=b"\n", seed=0, capacity=None, room=None):
        """k_field_chunks, k_field_link, k_linehash_chunks, k_linehash_link, k_scan_tiles, k_fieldhash_emit,
        k_fieldhash_finish: field_spans with the key of the field beside its span -> (summaries, keys, starts, sizes).  A
        summary is field_spans' dict with head and tail as (h, xl) of hash_lines, head_hashes (one per head position: the
        hash of the span's bytes in front of it) and tail_start_hash, tail_end_hash (None where the tail's field does not
        reach them).  keys is a numpy uint64 array shaped and filled like starts and sizes: `room` values that were all
        ones before the call, of which the call may write the first `capacity`."""
        import numpy as np
        nl, dl, field = _field_query_arguments(newline, delimiter, field)
        seed = int(seed)
        if seed < 0 or seed >= 2**64:
            raise ValueError("seed must not be negative and must fit 64 bits")
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        summaries = (FieldHashSummary * max(1, len(spans)))()
        heads = np.zeros(max(1, len(spans) * (field + 1)), dtype=np.uint64)
        head_hashes = np.zeros(max(1, len(spans) * (field + 1)), dtype=np.uint64)

        def call(keys, starts, sizes, capacity):
            self._check(lib().mi355x_bz2_field_hashes(self._h, arr, len(spans), nl, dl, field, seed, summaries,
                                                      heads.ctypes.data, head_hashes.ctypes.data, keys, starts, sizes, capacity))
        if capacity is None:
            call(None, None, None, 0)
            capacity = sum(s.count for s in summaries[:len(spans)])
        room = capacity if room is None else max(int(room), capacity)
        keys = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        starts = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        sizes = np.full(max(1, room), -1 - 2**62, dtype=np.int64)
        _with_device_copies("field_hashes", [keys, starts, sizes], lambda *device: call(*device, capacity))
        none = 2**64 - 1
        out = []
        for i, s in enumerate(summaries[:len(spans)]):
            at = i * (field + 1)
            out.append({**_field_summary_dict(s, heads[at:]),
                        "head_hashes": [int(v) for v in head_hashes[at:at + s.head_delims]],
                        "tail_start_hash": None if s.tail_field_start == none else int(s.tail_start_hash),
                        "tail_end_hash": None if s.tail_field_end == none else int(s.tail_end_hash),
                        "head": (int(s.head_hash), int(s.head_xl)), "tail": (int(s.tail_hash), int(s.tail_xl))})
        return out, keys[:room], starts[:room], sizes[:room]

    def field_numbers(self, spans, field, delimiter=b"\t", newline=b"\n", capacity=None, room=None):
        """k_field_chunks, k_field_link, k_scan_tiles, k_field_emit, k_field_sizes, k_field_numbers, k_field_texts:
        field_spans with the number of the field beside its span -> (summaries, numbers, starts, sizes).  A summary is
        field_spans' dict with head_texts (one (size, bytes) per head segment: the span's bytes between two head
        positions, at most field + 1 of them, the size saturated at 20 and at most 19 bytes kept) and tail_text (that of
        the tail line's field as far as the span reaches).  numbers is a numpy int64 array shaped and filled like starts
        and sizes: `room` values that were FIELD_NOT_A_NUMBER + 2 before the call, of which the call may write the first
        `capacity`: parse_field_number's value, FIELD_NOT_A_NUMBER, or FIELD_NUMBER_MISSING (not awk's strtod)."""
        import numpy as np
        nl, dl, field = _field_query_arguments(newline, delimiter, field)
        spans = [(int(o), int(n)) for o, n in spans]
        arr = (ByteSpan * max(1, len(spans)))(*[ByteSpan(o, n) for o, n in spans])
        summaries = (FieldSummary * max(1, len(spans)))()
        heads = np.zeros(max(1, len(spans) * (field + 1)), dtype=np.uint64)
        head_texts = (FieldText * max(1, len(spans) * (field + 1)))()
        tail_texts = (FieldText * max(1, len(spans)))()

        def call(numbers, starts, sizes, capacity):
            self._check(lib().mi355x_bz2_field_numbers(self._h, arr, len(spans), nl, dl, field, summaries, heads.ctypes.data,
                                                       head_texts, tail_texts, numbers, starts, sizes, capacity))
        if capacity is None:
            call(None, None, None, 0)
            capacity = sum(s.count for s in summaries[:len(spans)])
        room = capacity if room is None else max(int(room), capacity)
        numbers = np.full(max(1, room), FIELD_NOT_A_NUMBER + 2, dtype=np.int64)
        starts = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        sizes = np.full(max(1, room), -1 - 2**62, dtype=np.int64)
        _with_device_copies("field_numbers", [numbers, starts, sizes], lambda *device: call(*device, capacity))
        out = []
        for i, s in enumerate(summaries[:len(spans)]):
            at = i * (field + 1)
            listed = min(s.head_delims + 1, field + 1)
            out.append({**_field_summary_dict(s, heads[at:]),
                        "head_texts": [text.as_tuple() for text in head_texts[at:at + listed]],
                        "tail_text": tail_texts[i].as_tuple()})
        return out, numbers[:room], starts[:room], sizes[:room]

    def match_fields(self, values, keys, starts, sizes, base=0, seed=0, room=None, check=True):
        """k_field_match: is the field of every line one of `values`, byte for byte?  keys, starts and sizes are
        field_hashes' three arrays for n lines of the last batch's output (made under `seed`); start - base is a field's
        offset in that output -> flags: a numpy uint64 array of `room` words (default: n) that were all ones before the
        call, of which the call writes the first n: 1 where the line matches, 0 elsewhere.  The key only filters: a line
        whose key is a value's but whose bytes are not gives 0."""
        import numpy as np
        data, value_sizes, n_values = value_set(values, check=check)
        seed = int(seed)
        if seed < 0 or seed >= 2**64:
            raise ValueError("seed must not be negative and must fit 64 bits")
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        if keys.ndim != 1 or keys.shape != starts.shape or keys.shape != sizes.shape:
            raise ValueError("keys, starts and sizes must be one-dimensional and equally long")
        n = int(keys.size)
        room = n if room is None else max(int(room), n)
        flags = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        hosts = [np.resize(keys, max(1, n)), np.resize(starts, max(1, n)), np.resize(sizes, max(1, n)), flags]

        def call(d_keys, d_starts, d_sizes, d_flags):
            self._check(lib().mi355x_bz2_match_fields(self._h, data, value_sizes, n_values, seed, d_keys, d_starts, d_sizes, n,
                                                      int(base) % 2**64, d_flags))
        _with_device_copies("match_fields", hosts, call)
        return flags[:room]

    def match_fields_regex(self, regex, starts, sizes, base=0, room=None):
        """k_field_regex: does the field of every line match `regex` (compile_regex, or a pattern to compile)?  The field
        is to the pattern what a line's content is to match_lines: `^` and `$` anchor to the field's ends.  starts and
        sizes are field_spans' two arrays for n lines of the last batch's output; start - base is a field's offset in that
        output -> flags: a numpy uint64 array of `room` words (default: n) that were all ones before the call, of which
        the call writes the first n: 1 where the line matches, 0 elsewhere (a size < 0, a span outside the output)."""
        import numpy as np
        if not isinstance(regex, CompiledRegex):
            regex = compile_regex(regex)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        if starts.ndim != 1 or starts.shape != sizes.shape:
            raise ValueError("starts and sizes must be one-dimensional and equally long")
        n = int(starts.size)
        room = n if room is None else max(int(room), n)
        flags = np.full(max(1, room), 2**64 - 1, dtype=np.uint64)
        hosts = [np.resize(starts, max(1, n)), np.resize(sizes, max(1, n)), flags]

        def call(d_starts, d_sizes, d_flags):
            self._check(lib().mi355x_bz2_match_fields_regex(self._h, regex._h, d_starts, d_sizes, n, int(base) % 2**64, d_flags))
        _with_device_copies("match_fields_regex", hosts, call)
        return flags[:room]

    def output_device_ptr(self) -> int:
        return lib().mi355x_bz2_output_device(self._h) or 0

    def stream_ptr(self) -> int:
        return lib().mi355x_bz2_stream(self._h) or 0

    def device_memory(self) -> dict:
        """bytes of HBM this context holds: per-block scratch and output buffers"""
        scratch, output = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(lib().mi355x_bz2_device_memory(self._h, ctypes.byref(scratch), ctypes.byref(output)))
        return {"scratch_bytes": scratch.value, "output_bytes": output.value}

    def hold_output_until(self, hip_event: int, keepalive=None):
        """The next batch's output kernels wait for `hip_event` (e.g. torch.cuda.Event.cuda_event recorded behind a
        collective that reads output_device_ptr()); the event object must stay alive: pass it as `keepalive`."""
        self._output_hold = keepalive
        self._check(lib().mi355x_bz2_hold_output_until(self._h, hip_event))

    def copy_output_begin(self, offset: int, size: int):
        """Background D2H of the last batch's bytes; returns the ctypes buffer, valid after copy_output_end()."""
        buf = (ctypes.c_ubyte * max(1, size))()
        self._check(lib().mi355x_bz2_copy_output_begin(self._h, offset, size, buf))
        return buf

    def copy_output_begin_to(self, offset: int, size: int, host_ptr: int, keepalive=None):
        """The same into caller-owned (page-locked) host memory at address `host_ptr`; valid after copy_output_end()."""
        self._copy_ref = keepalive
        self._check(lib().mi355x_bz2_copy_output_begin(self._h, offset, size, ctypes.c_void_p(host_ptr)))

    def copy_output_end(self):
        self._check(lib().mi355x_bz2_copy_output_end(self._h))

    def copy_output(self, offset: int, size: int) -> bytes:
        buf = ctypes.create_string_buffer(max(1, size))
        self._check(lib().mi355x_bz2_copy_output(self._h, offset, size, buf))
        return buf.raw[:size]

    def pipeline_ms(self) -> float:
        """GPU time of the last batch between HIP events before its first and after its last kernel."""
        ms = ctypes.c_float(0)
        self._check(lib().mi355x_bz2_last_pipeline_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def timings(self) -> dict:
        t = Timings()
        self._check(lib().mi355x_bz2_last_timings(self._h, ctypes.byref(t)))
        return t.as_dict()

    def debug_stage(self, index: int, stage: int) -> bytes:
        if stage >= 3:      # k_hscan hand-off: 3 = group starts (u32 each), 4 = ScanMeta, 5 = selectors
            n = {3: 18048 * 4, 4: 32, 5: 32768}[stage]
        else:
            n = self.last_results[index]["bwt_length"] * (4 if stage == 1 else 1)
        buf = ctypes.create_string_buffer(max(1, n))
        self._check(lib().mi355x_bz2_debug_copy_stage(self._h, index, stage, buf, n))
        return buf.raw[:n]
