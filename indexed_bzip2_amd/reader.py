"""Host-side mirror of the reference's Python module (python/indexed_bzip2/indexed_bzip2.pyx:87-345).

Same names and argument meaning: open(), IndexedBzip2File(io.BufferedReader), IndexedBzip2FileRaw(io.RawIOBase) with
tell_compressed, block_offsets, set_block_offsets, block_offsets_complete, available_block_offsets, size,
join_threads.  The C++ ParallelBZ2Reader the Cython classes wrap is replaced by mi355x_bz2_reader_* (C ABI), whose
blocks are decoded on the GPU.  `parallelization` keeps the reference's meaning and default
(indexed_bzip2.pyx:293, 321, 340): 1 (default) = no parallelism, i.e. one block per GPU launch and -- like the serial
BZ2Reader that the reference selects for 1 -- the stream CRC of every end-of-stream block is verified
(BZ2Reader.hpp:406-416); 0 = as much as the machine wants (reference: all cores; here: the default batch of 512
blocks); N > 1 = N blocks per GPU batch, no stream-CRC check (ParallelBZ2Reader never checks it).  There is no CPU
reader: every value decodes on the GPU.

Threads: a reader (like a Decoder, and a mi355x_bz2_ctx in C) is used by one thread at a time -- its calls are not
serialised against one another, and the buffered position and a held result belong to that one caller.  Different readers
on different threads are independent, on the same GPU too: open one per worker thread.  The functions of buffers.py
(decompress, decompress_many, decompress_many_to_tensor, compress, compress_many) may be called from any thread; they
take turns on the device's kept context behind a lock.  The MI355X_BZ2_* environment switches are read while the library
runs, so os.environ must not be changed while another thread is inside it.  The *_to_tensor calls need torch's HIP
runtime to be the first in the process (import torch and touch the GPU before the first reader), on whichever thread.
tests/test_gpu_threads.py pins this.
"""
import ctypes
import builtins
import io
import os

from . import _native as N


def _has_valid_fileno(file):
    # indexed_bzip2.pyx:78-84
    try:
        fileno = file.fileno()
        return isinstance(fileno, int) and fileno >= 0
    except Exception:
        return False


def _is_file_object(file):
    # indexed_bzip2.pyx:69-76
    return all(hasattr(file, name) for name in ("read", "seekable", "seek", "tell"))


class _IndexedBzip2FileParallel:
    """Mirror of cdef class _IndexedBzip2FileParallel (indexed_bzip2.pyx:186-288)."""

    def __init__(self, file, parallelization=1, device=-1):
        if not isinstance(parallelization, int):
            raise TypeError(f"Parallelization argument must be an integer not '{parallelization}'!")
        self._h = ctypes.c_void_p()
        self._keepalive = None
        self._device = device
        L = N.lib()
        if isinstance(file, int):
            rc = L.mi355x_bz2_reader_open_fd(file, parallelization, device, ctypes.byref(self._h))
        elif _has_valid_fileno(file):
            rc = L.mi355x_bz2_reader_open_fd(file.fileno(), parallelization, device, ctypes.byref(self._h))
        elif _is_file_object(file):
            # pure-Python file object (the reference wraps it in PythonFileReader, filereader/Python.hpp:321-585):
            # the compressed bytes are pulled once; decoding needs them resident in HBM anyway
            pos = file.tell() if file.seekable() else None
            if pos is not None:
                file.seek(0)
            data = file.read()
            if pos is not None:
                file.seek(pos)
            rc = L.mi355x_bz2_reader_open_memory(data, len(data), parallelization, device, ctypes.byref(self._h))
        elif isinstance(file, (str, os.PathLike)):
            rc = L.mi355x_bz2_reader_open_path(os.fsencode(file), parallelization, device, ctypes.byref(self._h))
        else:
            raise Exception("Expected file name string, file descriptor integer, "
                            "or file-like object for ParallelBZ2Reader!")
        if rc != N.OK:
            self._h = ctypes.c_void_p()
            raise N.Bz2Error(rc)

    # -- helpers
    def _check(self, rc):
        if rc != N.OK:
            detail = N.lib().mi355x_bz2_reader_last_error(self._h).decode(errors="replace")
            if rc == 103:
                raise ValueError(detail or N.status_string(rc))
            raise N.Bz2Error(rc, detail)

    def _require(self):
        if not self._h:
            raise Exception("Invalid file object!")

    def _device_index(self):
        """The reader's device index for torch: the one it was opened with, or torch's current device."""
        import torch
        torch.cuda.init()
        return self._device if self._device >= 0 else torch.cuda.current_device()

    def _columns(self, query, take, dtypes, tensors):
        """Step 1 of a per-line query, then its take -> one array per column.  query(keep_on_device, n) is the native call
        that holds the columns and sets n, the number of lines; take(*destinations, n, on_device) copies their first n
        values.  The arrays are numpy arrays of `dtypes`, or with `tensors` torch.int64 tensors on the reader's device,
        which nothing reaches through the host."""
        n = ctypes.c_uint64()
        if not tensors:
            import numpy as np
            self._check(query(0, ctypes.byref(n)))
            out = [np.empty(n.value, dtype=dtype) for dtype in dtypes]
            self._check(take(*[column.ctypes.data if n.value else None for column in out], n.value, 0))
            return out
        import torch
        dev = self._device_index()
        self._check(query(1, ctypes.byref(n)))
        out = [torch.empty(n.value, dtype=torch.int64, device=f"cuda:{dev}") for _ in dtypes]
        if n.value:
            # the new tensors' memory may still be in use by work queued on torch's stream: the copy comes after it
            torch.cuda.current_stream(out[0].device).synchronize()
            self._check(take(*[ctypes.c_void_p(column.data_ptr()) for column in out], n.value, 1))
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        if self._h:
            N.lib().mi355x_bz2_reader_close(self._h)
            self._h = ctypes.c_void_p()

    def closed(self):
        return (not self._h) or bool(N.lib().mi355x_bz2_reader_closed(self._h))

    def seekable(self):
        self._require()
        return True

    def readinto(self, bytes_like):
        self._require()
        view = memoryview(bytes_like).cast("B")
        n = len(view)
        if n == 0:
            return 0
        buf = (ctypes.c_char * n).from_buffer(view)
        got = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_read(self._h, -1, buf, n, ctypes.byref(got)))
        return got.value

    def read_to_fd(self, fd, n=2**64 - 1):
        """read( fd, nullptr, n ): decode straight into a file descriptor (BZ2ReaderInterface.hpp:35-57)."""
        self._require()
        got = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_read(self._h, fd, None, n, ctypes.byref(got)))
        return got.value

    def seek(self, offset, whence=io.SEEK_SET):
        self._require()
        pos = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_seek(self._h, offset, whence, ctypes.byref(pos)))
        return pos.value

    def tell(self):
        self._require()
        return N.lib().mi355x_bz2_reader_tell(self._h)

    def size(self):
        self._require()
        s = ctypes.c_uint64()
        return s.value if N.lib().mi355x_bz2_reader_size(self._h, ctypes.byref(s)) else 0

    def tell_compressed(self):
        self._require()
        return N.lib().mi355x_bz2_reader_tell_compressed(self._h)

    def block_offsets_complete(self):
        self._require()
        return bool(N.lib().mi355x_bz2_reader_block_offsets_complete(self._h))

    def _offsets(self, fn):
        n = ctypes.c_uint64()
        self._check(fn(self._h, None, None, 0, ctypes.byref(n)))
        bits = (ctypes.c_uint64 * max(1, n.value))()
        byts = (ctypes.c_uint64 * max(1, n.value))()
        self._check(fn(self._h, bits, byts, n.value, ctypes.byref(n)))
        return {bits[i]: byts[i] for i in range(n.value)}

    def block_offsets(self):
        self._require()
        return self._offsets(N.lib().mi355x_bz2_reader_block_offsets)

    def available_block_offsets(self):
        self._require()
        return self._offsets(N.lib().mi355x_bz2_reader_available_block_offsets)

    def set_block_offsets(self, offsets):
        self._require()
        items = sorted(dict(offsets).items())
        n = len(items)
        bits = (ctypes.c_uint64 * max(1, n))(*[k for k, _ in items])
        byts = (ctypes.c_uint64 * max(1, n))(*[v for _, v in items])
        self._check(N.lib().mi355x_bz2_reader_set_block_offsets(self._h, bits, byts, n))

    def join_threads(self):
        self._require()
        self._check(N.lib().mi355x_bz2_reader_join_threads(self._h))

    def read_ranges_into(self, offsets, sizes, out):
        """pread of many ranges at once: range i = `sizes[i]` bytes at decoded offset `offsets[i]`, written to `out` at
        sum(sizes[:i]).  `out` is a writable contiguous host buffer, or a contiguous torch.uint8 tensor on the reader's
        device (the bytes then never pass through the host).  Every block the ranges need is decoded once; the read
        position is not moved.  Returns the bytes read per range (numpy uint64; short only at the end of the file; the
        bytes of `out` behind them are left as they were)."""
        import numpy as np
        self._require()
        offsets = [int(o) for o in offsets]
        sizes = [int(s) for s in sizes]
        if len(offsets) != len(sizes):
            raise ValueError(f"{len(offsets)} offsets but {len(sizes)} sizes")
        if any(o < 0 for o in offsets) or any(s < 0 for s in sizes):
            raise ValueError("offsets and sizes must not be negative")
        n = len(offsets)
        total = sum(sizes)
        if getattr(out, "is_cuda", False):
            import torch
            if out.dtype != torch.uint8 or not out.is_contiguous():
                raise ValueError("a device destination must be a contiguous torch.uint8 tensor")
            capacity, device = out.numel(), 1
            # the tensor may still be written by work queued on torch's stream (a fill): the gather comes after it
            torch.cuda.current_stream(out.device).synchronize()
            dst = ctypes.c_void_p(out.data_ptr())
        else:
            view = memoryview(out).cast("B")
            if view.readonly:
                raise ValueError("the destination buffer is read-only")
            capacity, device = len(view), 0
            dst = (ctypes.c_char * max(1, capacity)).from_buffer(view) if capacity > 0 else None
        if capacity < total:
            raise ValueError(f"the destination holds {capacity} bytes, the ranges need {total}")
        offs = (ctypes.c_uint64 * max(1, n))(*offsets)
        lens = (ctypes.c_uint64 * max(1, n))(*sizes)
        got = (ctypes.c_uint64 * max(1, n))()
        self._check(N.lib().mi355x_bz2_reader_read_ranges(self._h, offs, lens, n, dst, device, got))
        return np.frombuffer(got, dtype=np.uint64, count=n).copy()

    def read_ranges(self, ranges):
        """[(offset, size), ...] -> one bytes object per range, as long as what the file holds of it."""
        ranges = [(int(o), int(s)) for o, s in ranges]
        if any(o < 0 or s < 0 for o, s in ranges):
            raise ValueError("offsets and sizes must not be negative")
        out = bytearray(sum(s for _, s in ranges))
        got = self.read_ranges_into([o for o, _ in ranges], [s for _, s in ranges], out)
        result, at = [], 0
        for (_, size), n in zip(ranges, got):
            result.append(bytes(out[at:at + int(n)]))
            at += size
        return result

    # -- line access: `newline` is one delimiter byte; line k (0-based) starts behind the k-th delimiter, the last line
    # is the unterminated tail (possibly empty), and a range (first, count) holds its lines with their delimiters
    @staticmethod
    def _newline(newline):
        if not isinstance(newline, (bytes, bytearray)) or len(newline) != 1:
            raise ValueError("newline must be exactly one byte, e.g. b'\\n'")
        return newline[0]

    @staticmethod
    def _u64(values, what):
        values = [int(v) for v in values]
        if any(v < 0 for v in values):
            raise ValueError(f"{what} must not be negative")
        if any(v >= 2**64 for v in values):
            raise ValueError(f"{what} must fit 64 bits")
        return values, (ctypes.c_uint64 * max(1, len(values)))(*values)

    def line_offsets(self, newline=b"\n"):
        """The line index {decoded byte offset of a block's first byte: delimiters in front of it}, one entry per data
        block and {size: number of delimiters} at the end; {0: 0} for an empty file.  Built on the GPU when the reader
        does not hold it for this `newline` (the block map is completed first): every block is decoded once, counted
        where it lies, and only the counts come back.  Positionless."""
        self._require()
        nl = self._newline(newline)
        fn = N.lib().mi355x_bz2_reader_line_offsets
        n = ctypes.c_uint64()
        self._check(fn(self._h, nl, None, None, 0, ctypes.byref(n)))
        byts = (ctypes.c_uint64 * max(1, n.value))()
        lines = (ctypes.c_uint64 * max(1, n.value))()
        self._check(fn(self._h, nl, byts, lines, n.value, ctypes.byref(n)))
        return {byts[i]: lines[i] for i in range(n.value)}

    def set_line_offsets(self, offsets, newline=b"\n"):
        """Import a line index (line_offsets() of an earlier session, read_line_offsets); the block map must be complete
        (set_block_offsets).  ValueError if it does not fit the block map."""
        self._require()
        nl = self._newline(newline)
        items = sorted(dict(offsets).items())
        _, byts = self._u64([k for k, _ in items], "offsets")
        _, lines = self._u64([v for _, v in items], "line numbers")
        self._check(N.lib().mi355x_bz2_reader_set_line_offsets(self._h, nl, byts, lines, len(items)))

    def count_lines(self, newline=b"\n"):
        """The number of `newline` bytes in the decoded file (the last value of line_offsets)."""
        offsets = self.line_offsets(newline)
        return max(offsets.values())

    def line_starts(self, lines, newline=b"\n"):
        """Decoded byte offset at which each of the given lines starts (numpy uint64); the size of the file for line
        numbers beyond the last line.  Only the blocks that hold one of these line starts are decoded."""
        import numpy as np
        self._require()
        nl = self._newline(newline)
        lines, arr = self._u64(lines, "line numbers")
        out = (ctypes.c_uint64 * max(1, len(lines)))()
        self._check(N.lib().mi355x_bz2_reader_line_starts(self._h, nl, arr, len(lines), out))
        return np.frombuffer(out, dtype=np.uint64, count=len(lines)).copy()

    def _read_line_ranges(self, ranges, newline, on_device):
        """Step 1 (mi355x_bz2_reader_read_line_ranges): returns the byte size of every range."""
        self._require()
        nl = self._newline(newline)
        ranges = [(int(f), int(c)) for f, c in ranges]
        if any(f < 0 or c < 0 for f, c in ranges):
            raise ValueError("line numbers and counts must not be negative")
        _, first = self._u64([f for f, _ in ranges], "line numbers")
        _, count = self._u64([min(c, 2**64 - 1) for _, c in ranges], "counts")
        sizes = (ctypes.c_uint64 * max(1, len(ranges)))()
        total = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_read_line_ranges(self._h, nl, first, count, len(ranges),
                                                                1 if on_device else 0, sizes, ctypes.byref(total)))
        return [sizes[i] for i in range(len(ranges))], total.value

    def read_line_ranges(self, ranges, newline=b"\n"):
        """[(first line, number of lines), ...] -> one bytes object per range: the lines with their delimiters; what the
        file holds of them if the range reaches beyond the last line; b"" if it starts beyond it.  Every block the
        ranges need is decoded once, the lines are found on the GPU, and only their bytes are copied out.  Builds the
        line index first if the reader does not hold one for `newline`.  Positionless."""
        sizes, total = self._read_line_ranges(ranges, newline, False)
        out = bytearray(total)
        dst = (ctypes.c_char * max(1, total)).from_buffer(out) if total > 0 else None
        self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, dst, 0))
        del dst
        result, at = [], 0
        for size in sizes:
            result.append(bytes(out[at:at + size]))
            at += size
        return result

    def read_lines(self, first, count=1, newline=b"\n"):
        """`count` lines from line `first` (0-based) as one bytes object, delimiters included."""
        return self.read_line_ranges([(first, count)], newline)[0]

    def read_line_ranges_to_tensor(self, ranges, newline=b"\n"):
        """read_line_ranges into ONE contiguous torch.uint8 tensor on the reader's device -> (data, offsets): range i is
        ``data[offsets[i]:offsets[i + 1]]``; `offsets` is an int64 CPU tensor of n + 1 boundaries.  The bytes never pass
        through the host."""
        import torch
        dev = self._device_index()
        sizes, total = self._read_line_ranges(ranges, newline, True)
        data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
        if total:
            # the new tensor's memory may still be in use by work queued on torch's stream: the copy comes after it
            torch.cuda.current_stream(data.device).synchronize()
        self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, ctypes.c_void_p(data.data_ptr()) if total else None, 1))
        bounds = [0]
        for size in sizes:
            bounds.append(bounds[-1] + size)
        return data, torch.tensor(bounds, dtype=torch.int64)

    # -- search: a match of `pattern` (1 to 256 bytes) is every offset p with data[p:p + len(pattern)] == pattern,
    # start <= p and p + len(pattern) <= end; start and end are clipped to the decoded size.  ignore_case=True (keyword
    # only, on every search and grep method) compares data[p:p + len(pattern)].lower() with pattern.lower() instead: the
    # ASCII letters fold on the GPU, every other byte -- 0x80 to 0xFF included -- must be equal (LC_ALL=C grep -i)
    @staticmethod
    def _flags(ignore_case):
        return N.SEARCH_IGNORE_CASE if ignore_case else 0

    @staticmethod
    def _pattern(pattern):
        pattern = bytes(memoryview(pattern))     # TypeError for what is not bytes-like
        if not 1 <= len(pattern) <= 256:
            raise ValueError(f"the pattern must have 1 to 256 bytes, not {len(pattern)}")
        return pattern

    def _search(self, pattern, start, end, limit, ignore_case=False):
        """Step 1 (mi355x_bz2_reader_search_ex): the number of matches (limit 0), or of the positions now held."""
        self._require()
        pattern = self._pattern(pattern)
        start, end = int(start), 2**64 - 1 if end is None else int(end)
        if start < 0 or end < 0:
            raise ValueError("start and end must not be negative")
        n = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_search_ex(self._h, pattern, len(pattern), self._flags(ignore_case),
                                                        min(start, 2**64 - 1), min(end, 2**64 - 1), limit, ctypes.byref(n)))
        return n.value

    def count_matches(self, pattern, start=0, end=None, *, ignore_case=False):
        """How often the byte string `pattern` occurs in data[start:end] of the decoded file.  Occurrences that overlap
        each other all count -- b"abab" occurs 3 times in b"abababab" -- unlike bytes.count, which says 2.  Every block
        that intersects the range is decoded once, the matches are found on the GPU and only their number leaves it.
        ignore_case=True: the ASCII letters of pattern and data match in either case.  Positionless."""
        return self._search(pattern, start, end, 0, ignore_case)

    def find_all(self, pattern, start=0, end=None, limit=None, *, ignore_case=False):
        """The offsets in the decoded file of the occurrences of `pattern` in data[start:end] (numpy uint64, ascending),
        at most `limit` of them (None: all).  With a limit, no launch is started once it has been reached.  Overlapping
        occurrences as in count_matches.  Positionless."""
        import numpy as np
        if limit is not None and int(limit) < 0:
            raise ValueError("limit must not be negative")
        if limit is not None and int(limit) == 0:
            self._pattern(pattern)
            return np.empty(0, dtype=np.uint64)
        n = self._search(pattern, start, end, 2**64 - 1 if limit is None else min(int(limit), 2**64 - 1), ignore_case)
        out = (ctypes.c_uint64 * max(1, n))()
        self._check(N.lib().mi355x_bz2_reader_take_matches(self._h, out, n))
        return np.frombuffer(out, dtype=np.uint64, count=n).copy()

    def find(self, pattern, start=0, end=None, *, ignore_case=False):
        """The offset of the first occurrence of `pattern` in data[start:end], or -1: find_all with limit=1."""
        first = self.find_all(pattern, start, end, 1, ignore_case=ignore_case)
        return int(first[0]) if len(first) else -1

    # -- grep: the lines that hold a match.  A match belongs to the line of its first byte (the pattern may contain the
    # delimiter); start and end bound the matches, not the lines, which always come whole
    def line_numbers(self, offsets, newline=b"\n"):
        """The 0-based number of the line that holds each decoded byte offset (numpy uint64): the number of `newline`
        bytes in front of it, the inverse of line_starts.  Offsets at or beyond the size give the number of delimiters
        in the file.  Only the blocks that hold one of the offsets are decoded, the delimiters are counted on the GPU
        and only the numbers come back.  Builds the line index first if the reader does not hold one for `newline`.
        Positionless."""
        import numpy as np
        self._require()
        nl = self._newline(newline)
        if isinstance(offsets, np.ndarray) and offsets.dtype == np.uint64:
            values = np.ascontiguousarray(offsets).ravel()
        else:
            values, _ = self._u64(offsets, "offsets")
            values = np.array(values, dtype=np.uint64)
        out = np.empty(len(values), dtype=np.uint64)
        as_u64p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if len(a) else None
        self._check(N.lib().mi355x_bz2_reader_line_numbers(self._h, nl, as_u64p(values), len(values), as_u64p(out)))
        return out

    def _grep_arguments(self, pattern, start, end, newline, any_of=False):
        pattern = N.pattern_set(pattern) if any_of else self._pattern(pattern)
        nl = self._newline(newline)
        start, end = int(start), 2**64 - 1 if end is None else int(end)
        if start < 0 or end < 0:
            raise ValueError("start and end must not be negative")
        return pattern, nl, start, end

    def _grep(self, pattern, start, end, limit, newline, on_device, any_of=False, ignore_case=False):
        """Step 1 (mi355x_bz2_reader_grep_ex, or _grep_set_ex for a set of patterns) and the numbers and sizes of the held lines
        (_take_grep): (numbers, sizes, total bytes); with limit 0 nothing is held and the number of matching lines comes
        back instead."""
        import numpy as np
        self._require()
        pattern, nl, start, end = self._grep_arguments(pattern, start, end, newline, any_of)
        n, total = ctypes.c_uint64(), ctypes.c_uint64()
        if any_of:
            data, sizes, k = pattern
            self._check(N.lib().mi355x_bz2_reader_grep_set_ex(self._h, data, sizes, k, self._flags(ignore_case), nl,
                                                              min(start, 2**64 - 1), min(end, 2**64 - 1), limit,
                                                              1 if on_device else 0, ctypes.byref(n), ctypes.byref(total)))
        else:
            self._check(N.lib().mi355x_bz2_reader_grep_ex(self._h, pattern, len(pattern), self._flags(ignore_case), nl,
                                                          min(start, 2**64 - 1), min(end, 2**64 - 1), limit,
                                                          1 if on_device else 0, ctypes.byref(n), ctypes.byref(total)))
        if limit == 0:
            return n.value
        numbers = (ctypes.c_uint64 * max(1, n.value))()
        sizes = (ctypes.c_uint64 * max(1, n.value))()
        self._check(N.lib().mi355x_bz2_reader_take_grep(self._h, numbers, sizes, n.value))
        return (np.frombuffer(numbers, dtype=np.uint64, count=n.value).copy(), [sizes[i] for i in range(n.value)],
                total.value)

    @staticmethod
    def _line_limit(limit):
        if limit is not None and int(limit) < 0:
            raise ValueError("limit must not be negative")
        return 2**64 - 1 if limit is None else min(int(limit), 2**64 - 1)

    def count_matching_lines(self, pattern, start=0, end=None, newline=b"\n", *, ignore_case=False):
        """The number of distinct lines that hold an occurrence of `pattern` in data[start:end] (`grep -c -F`, with
        ignore_case `grep -c -F -i`)."""
        return self._grep(pattern, start, end, 0, newline, False, False, ignore_case)

    def grep(self, pattern, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """The lines that hold an occurrence of `pattern` in data[start:end] (`grep -n -F`) -> (numbers, lines): the
        0-based line numbers (numpy uint64, strictly ascending) and one bytes object per line, whole and with its
        delimiter (the unterminated tail as it is), at most `limit` lines (None: all).  An occurrence belongs to the
        line of its first byte; start and end bound the occurrences, not the lines.  Three passes on the GPU: the
        search, the line numbers of the matches (k_rank_byte), and the lines themselves; only numbers, sizes and the
        lines' bytes leave it.  Releases matches and line ranges held by earlier calls.  ignore_case=True
        is `grep -n -F -i` in the C locale: it changes which occurrences the search pass finds and nothing else.
        Positionless."""
        return self._grep_lines(pattern, start, end, limit, newline, False, ignore_case)

    def _grep_lines(self, pattern, start, end, limit, newline, any_of, ignore_case=False):
        import numpy as np
        limit = self._line_limit(limit)
        if limit == 0:                                 # nothing is asked for: the arguments are checked, nothing runs
            self._require()
            self._grep_arguments(pattern, start, end, newline, any_of)
            return np.empty(0, dtype=np.uint64), []
        numbers, sizes, total = self._grep(pattern, start, end, limit, newline, False, any_of, ignore_case)
        out = bytearray(total)
        dst = (ctypes.c_char * max(1, total)).from_buffer(out) if total > 0 else None
        self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, dst, 0))
        del dst
        lines, at = [], 0
        for size in sizes:
            lines.append(bytes(out[at:at + size]))
            at += size
        return numbers, lines

    def grep_to_tensor(self, pattern, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """grep into ONE contiguous torch.uint8 tensor on the reader's device -> (numbers, data, offsets), data and
        offsets laid out as read_line_ranges_to_tensor: line i is ``data[offsets[i]:offsets[i + 1]]``.  The lines' bytes
        never pass through the host."""
        return self._grep_tensor(pattern, start, end, limit, newline, False, ignore_case)

    def _grep_tensor(self, pattern, start, end, limit, newline, any_of, ignore_case=False):
        import numpy as np
        import torch
        limit = self._line_limit(limit)
        self._require()
        self._grep_arguments(pattern, start, end, newline, any_of)
        dev = self._device_index()
        if limit == 0:
            numbers, sizes, total = np.empty(0, dtype=np.uint64), [], 0
        else:
            numbers, sizes, total = self._grep(pattern, start, end, limit, newline, True, any_of, ignore_case)
        data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
        if total:
            # the new tensor's memory may still be in use by work queued on torch's stream: the copy comes after it
            torch.cuda.current_stream(data.device).synchronize()
        if limit != 0:
            self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, ctypes.c_void_p(data.data_ptr()) if total else None, 1))
        bounds = [0]
        for size in sizes:
            bounds.append(bounds[-1] + size)
        return numbers, data, torch.tensor(bounds, dtype=torch.int64)

    # -- grep for a regular expression: a line matches iff re.search(pattern, content, re.DOTALL) finds a match in its
    # content (the line without its delimiter; the unterminated tail is a line only if it is non-empty).  The pattern is
    # compiled on the host to a DFA of at most 64 states (N.compile_regex names the syntax), the GPU runs it over the whole
    # decoded file, and the rank and line passes are grep's.  There is no start / end
    @staticmethod
    def _regex(pattern, ignore_case):
        if isinstance(pattern, N.CompiledRegex):
            if ignore_case and not pattern.ignore_case:
                raise ValueError("ignore_case is a property of the compiled regex: compile_regex(pattern, ignore_case=True)")
            return pattern
        return N.compile_regex(pattern, ignore_case)

    def _grep_regex(self, regex, limit, nl, on_device):
        """Step 1 (mi355x_bz2_reader_grep_regex) and the numbers and sizes of the held lines, as _grep."""
        import numpy as np
        n, total = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_grep_regex(self._h, regex._h, nl, limit, 1 if on_device else 0,
                                                         ctypes.byref(n), ctypes.byref(total)))
        if limit == 0:
            return n.value
        numbers = (ctypes.c_uint64 * max(1, n.value))()
        sizes = (ctypes.c_uint64 * max(1, n.value))()
        self._check(N.lib().mi355x_bz2_reader_take_grep(self._h, numbers, sizes, n.value))
        return (np.frombuffer(numbers, dtype=np.uint64, count=n.value).copy(), [sizes[i] for i in range(n.value)],
                total.value)

    def count_matching_lines_regex(self, pattern, newline=b"\n", *, ignore_case=False):
        """The number of lines whose content matches the regular expression `pattern` (`grep -c`, with ignore_case
        `grep -c -i`): bytes-like, or compiled by compile_regex.  One pass on the GPU, only counts leave it."""
        self._require()
        regex, nl = self._regex(pattern, ignore_case), self._newline(newline)
        return self._grep_regex(regex, 0, nl, False)

    def grep_regex(self, pattern, limit=None, newline=b"\n", *, ignore_case=False):
        """The lines whose content matches the regular expression `pattern` (`bzgrep -n PATTERN`) -> (numbers, lines), as
        grep returns them: 0-based line numbers (numpy uint64, strictly ascending) and one bytes object per line, whole
        and with its delimiter, at most `limit` lines (None: all).  `pattern` is bytes-like or compiled by compile_regex;
        a pattern outside the supported syntax is a ValueError before anything is launched.  The whole file is searched.
        Positionless; releases matches and line ranges held by earlier calls."""
        import numpy as np
        limit = self._line_limit(limit)
        self._require()
        regex, nl = self._regex(pattern, ignore_case), self._newline(newline)
        if limit == 0:                                 # nothing is asked for: the arguments are checked, nothing runs
            return np.empty(0, dtype=np.uint64), []
        numbers, sizes, total = self._grep_regex(regex, limit, nl, False)
        out = bytearray(total)
        dst = (ctypes.c_char * max(1, total)).from_buffer(out) if total > 0 else None
        self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, dst, 0))
        del dst
        lines, at = [], 0
        for size in sizes:
            lines.append(bytes(out[at:at + size]))
            at += size
        return numbers, lines

    def grep_regex_to_tensor(self, pattern, limit=None, newline=b"\n", *, ignore_case=False):
        """grep_regex into ONE contiguous torch.uint8 tensor on the reader's device -> (numbers, data, offsets), as
        grep_to_tensor."""
        import numpy as np
        import torch
        limit = self._line_limit(limit)
        self._require()
        regex, nl = self._regex(pattern, ignore_case), self._newline(newline)
        dev = self._device_index()
        if limit == 0:
            numbers, sizes, total = np.empty(0, dtype=np.uint64), [], 0
        else:
            numbers, sizes, total = self._grep_regex(regex, limit, nl, True)
        data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
        if total:
            torch.cuda.current_stream(data.device).synchronize()
        if limit != 0:
            self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, ctypes.c_void_p(data.data_ptr()) if total else None, 1))
        bounds = [0]
        for size in sizes:
            bounds.append(bounds[-1] + size)
        return numbers, data, torch.tensor(bounds, dtype=torch.int64)

    # -- line hashes: one 61-bit polynomial hash per line (N.line_hash says which), computed where the decoded bytes lie.
    # Lines are numbered as grep numbers them; a non-empty unterminated tail is the last line.  Equal contents have equal
    # hashes; two distinct contents of at most L bytes have equal hashes for at most L of the 2^61 bases a seed can give,
    # so "distinct" below means "of distinct hash", and a second seed is an independent check
    def _line_hash_arguments(self, first, count, newline, seed):
        self._require()
        nl = self._newline(newline)
        (first, seed), _ = self._u64([first, seed], "first and seed")
        (count,), _ = self._u64([2**64 - 1 if count is None else count], "count")
        return nl, first, count, seed

    def _line_hashes(self, first, count, newline, seed, tensors):
        nl, first, count, seed = self._line_hash_arguments(first, count, newline, seed)
        L = N.lib()
        return self._columns(lambda keep, n: L.mi355x_bz2_reader_line_hashes(self._h, nl, seed, first, count, keep, n),
                             lambda *to: L.mi355x_bz2_reader_take_line_hashes(self._h, *to), ("uint64",), tensors)[0]

    def line_hashes(self, first=0, count=None, newline=b"\n", seed=0):
        """The hashes of lines [first, first + count) (count None: to the last line; clipped there) -> numpy uint64, one
        value below 2^61 per line, equal to line_hash(content, seed).  Only the blocks that hold those lines are decoded,
        each once; the hashes are computed on the GPU and 8 bytes per line come back.  Builds the line index first if
        the reader does not hold one for `newline`.  Positionless."""
        return self._line_hashes(first, count, newline, seed, False)

    def line_hashes_to_tensor(self, first=0, count=None, newline=b"\n", seed=0):
        """line_hashes as a torch.int64 tensor on the reader's device; the hashes never pass through the host.  A hash
        is below 2^61, so torch.unique, sort and isin order and compare it as the unsigned value."""
        return self._line_hashes(first, count, newline, seed, True)

    def _distinct_lines(self, newline, seed, want_numbers):
        nl, _, _, seed = self._line_hash_arguments(0, None, newline, seed)
        n = ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_distinct_lines(self._h, nl, seed, 1 if want_numbers else 0, ctypes.byref(n)))
        return n.value

    def count_distinct_lines(self, newline=b"\n", seed=0):
        """The number of distinct lines (`sort -u | wc -l`): of distinct hashes, see above.  The whole file is hashed
        and the hashes are sorted on the GPU; one number comes back."""
        return self._distinct_lines(newline, seed, False)

    def first_occurrences(self, newline=b"\n", seed=0):
        """The numbers of the lines that are the first of their content (`awk '!seen[$0]++'`) -> numpy uint64, ascending,
        ready for read_line_ranges([(k, 1) for k in ...])."""
        import numpy as np
        n = self._distinct_lines(newline, seed, True)
        out = np.empty(n, dtype=np.uint64)
        self._check(N.lib().mi355x_bz2_reader_take_distinct_lines(
            self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if n else None, n))
        return out

    # -- fields: where field j of every line lies and what it holds.  A line's content (the line without `newline`) is
    # split at every `delimiter` byte exactly as bytes.split(delimiter) splits it; field j, 0-based, is missing in a line
    # with fewer than j delimiters.  There is no quoting and no escaping: this is `cut -f` / `awk -F`, not a CSV parser.
    # Lines are numbered as line_hashes numbers them; a non-empty unterminated tail is the last line
    def _field_arguments(self, field, first, count, delimiter, newline):
        self._require()
        nl = self._newline(newline)
        if not isinstance(delimiter, (bytes, bytearray)) or len(delimiter) != 1:
            raise ValueError("delimiter must be exactly one byte, e.g. b'\\t'")
        if delimiter[0] == nl:
            raise ValueError("delimiter and newline must differ")
        field = int(field)
        if field < 0 or field > 1023:
            raise ValueError("field must be between 0 and 1023")
        (first,), _ = self._u64([first], "first")
        (count,), _ = self._u64([2**64 - 1 if count is None else count], "count")
        return nl, delimiter[0], field, first, count

    # -- quote=: None, or one byte that differs from `delimiter` and `newline`.  Within a line every quote byte toggles
    # "inside quotes" and only the delimiters outside part the line, so a doubled quote inside a quoted field needs no rule
    # of its own and an unbalanced quote makes the rest of the line one field.  `newline` ALWAYS ends the line and the quote
    # state: a quoted field cannot hold a newline, and lines keep their numbers.  The field reported is the CONTENT: a raw
    # field of 2 bytes or more whose first and last bytes are both the quote loses these two; `""` is the empty field, a
    # lone `"` stays.  Doubled quotes inside stay doubled -- spans of the file come back, no byte is rewritten -- and there
    # are no backslash escapes.  field_spans, read_fields, read_columns and their tensor forms take it
    @staticmethod
    def _quote_argument(quote, nl, dl):
        if quote is None:
            return None
        if not isinstance(quote, (bytes, bytearray, memoryview)) or len(bytes(quote)) != 1:
            raise ValueError("quote must be None or exactly one byte, e.g. b'\"'")
        quote = bytes(quote)
        if quote[0] == nl or quote[0] == dl:
            raise ValueError("quote must differ from delimiter and newline")
        return quote[0]

    def _field_spans(self, field, first, count, delimiter, newline, tensors, quote=None):
        nl, dl, field, first, count = self._field_arguments(field, first, count, delimiter, newline)
        q = self._quote_argument(quote, nl, dl)
        L = N.lib()
        if q is None:
            launch = lambda keep, n: L.mi355x_bz2_reader_field_spans(self._h, nl, dl, field, first, count, keep, n)
        else:
            launch = lambda keep, n: L.mi355x_bz2_reader_field_spans_quoted(self._h, nl, dl, field, first, count, keep, n, q)
        return tuple(self._columns(launch, lambda *to: L.mi355x_bz2_reader_take_field_spans(self._h, *to), ("uint64", "int64"), tensors))

    def field_spans(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """Where field `field` (0-based, at most 1023) lies in lines [first, first + count) (count None: to the last
        line; clipped there) -> (starts numpy uint64, sizes numpy int64), one pair per line: data[start:start + size] ==
        content.split(delimiter)[field].  A line with fewer fields has size -1 and start = the offset at which its
        content ends.  No quoting, no escaping: `cut -f`, not a CSV parser.  Only the blocks that hold those lines are
        decoded, each once; the spans are computed on the GPU and 16 bytes per line come back.  Builds the line index
        first if the reader does not hold one for `newline`.  Positionless.

        With quote=b'"' (one byte, not `delimiter` or `newline`) delimiters inside quotes do not part the line and the
        span is the field's content, without an enclosing pair of quotes; doubled quotes inside stay doubled, and
        `newline` still ends every line: a quoted field cannot hold one."""
        return self._field_spans(field, first, count, delimiter, newline, False, quote)

    def field_spans_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """field_spans as two torch.int64 tensors (starts, sizes) on the reader's device; nothing passes through the
        host.  A start is below 2^63, so int64 holds it as it is."""
        return self._field_spans(field, first, count, delimiter, newline, True, quote)

    def _read_fields(self, field, first, count, delimiter, newline, make, quote=None):
        """field_spans, then the existing read_ranges over the present fields; make(total) -> (destination, pointer,
        is_device).  Returns (sizes numpy int64, bounds numpy int64 of n + 1, destination)."""
        import numpy as np
        starts, sizes = self.field_spans(field, first, count, delimiter, newline, quote=quote)
        n = len(starts)
        lengths = np.maximum(sizes, 0).astype(np.uint64)
        bounds = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lengths, out=bounds[1:])
        out, dst, device = make(int(bounds[-1]))
        if n:
            got = np.empty(n, dtype=np.uint64)
            u64p = ctypes.POINTER(ctypes.c_uint64)
            self._check(N.lib().mi355x_bz2_reader_read_ranges(self._h, starts.ctypes.data_as(u64p), lengths.ctypes.data_as(u64p),
                                                               n, dst, device, got.ctypes.data_as(u64p)))
        return sizes, bounds, out

    def read_fields(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """Field `field` of lines [first, first + count) -> a list with one bytes object per line, content.split(
        delimiter)[field], and None where the line has no such field.  No quoting, no escaping: `cut -f`, not a CSV
        parser.  field_spans finds the fields on the GPU; then the blocks that hold them are decoded a second time and
        only the fields' bytes are copied out.  Positionless.  read_columns gives the same, for several fields, from one
        decode.  quote= as for field_spans: the fields' contents, their doubled quotes kept."""
        def make(total):
            out = bytearray(total)
            return out, ((ctypes.c_char * total).from_buffer(out) if total else None), 0
        sizes, bounds, out = self._read_fields(field, first, count, delimiter, newline, make, quote)
        data = bytes(out)
        return [data[bounds[i]:bounds[i + 1]] if sizes[i] >= 0 else None for i in range(len(sizes))]

    def read_fields_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """read_fields into ONE contiguous torch.uint8 tensor on the reader's device -> (data, offsets) as
        read_line_ranges_to_tensor shapes them: line i's field is ``data[offsets[i]:offsets[i + 1]]``, `offsets` an
        int64 CPU tensor of n + 1 boundaries; a missing field has size 0 (field_spans tells it from an empty one).  The
        fields' bytes never pass through the host.  read_columns_to_tensor gives the bytes from one decode, with offsets
        and sizes on the device."""
        import torch
        nl, dl, _, _, _ = self._field_arguments(field, first, count, delimiter, newline)    # refused before the GPU is touched
        self._quote_argument(quote, nl, dl)
        dev = self._device_index()

        def make(total):
            data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
            if total:
                # the new tensor's memory may still be in use by work queued on torch's stream: the gather comes after it
                torch.cuda.current_stream(data.device).synchronize()
            return data, (ctypes.c_void_p(data.data_ptr()) if total else None), 1
        _, bounds, data = self._read_fields(field, first, count, delimiter, newline, make, quote)
        return data, torch.from_numpy(bounds)

    # -- field columns: the bytes of several fields of every line from ONE decode, each column packed on the GPU
    def _column_arguments(self, fields, first, count, delimiter, newline, quote=None):
        if isinstance(fields, (str, bytes, bytearray)):
            raise TypeError("fields must be a sequence of field numbers")
        fields = list(fields)
        if not 1 <= len(fields) <= 16:
            raise ValueError("fields must name 1 to 16 fields")
        nl = dl = first_ = count_ = None
        checked = []
        for field in fields:
            nl, dl, field, first_, count_ = self._field_arguments(field, first, count, delimiter, newline)
            checked.append(field)
        return nl, dl, checked, first_, count_, self._quote_argument(quote, nl, dl)

    def _field_columns(self, fields, first, count, delimiter, newline, quote=None):
        """mi355x_bz2_reader_field_columns -> (the number of lines, the bytes of every column); the columns are held."""
        nl, dl, fields, first, count, q = self._column_arguments(fields, first, count, delimiter, newline, quote)
        numbers = (ctypes.c_uint32 * len(fields))(*fields)
        n = ctypes.c_uint64()
        totals = (ctypes.c_uint64 * len(fields))()
        if q is None:
            self._check(N.lib().mi355x_bz2_reader_field_columns(self._h, nl, dl, numbers, len(fields), first, count, 1, ctypes.byref(n),
                                                                totals))
        else:
            self._check(N.lib().mi355x_bz2_reader_field_columns_quoted(self._h, nl, dl, numbers, len(fields), first, count, 1,
                                                                       ctypes.byref(n), totals, q))
        return n.value, list(totals)

    def read_columns_to_tensor(self, fields, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """The fields `fields` (1 to 16 field numbers, each at most 1023; one may be named twice) of lines [first, first +
        count) -> a list with one (data, offsets, sizes) per entry of `fields`, all on the reader's device: `data` a
        torch.uint8 tensor of the field's bytes packed in line order, `offsets` torch.int64 of n + 1 boundaries and `sizes`
        torch.int64 of n: ``data[offsets[i]:offsets[i + 1]] == content.split(delimiter)[field]``, and sizes[i] == -1 with
        an empty slice where line i has fewer fields.  Every needed block is decoded once, whatever the number of fields
        -- but for the few blocks that hold a line crossing a launch seam --, the GPU copies the fields out of the launch
        that found them, and nothing per line passes through the host.  No quoting, no escaping: `cut -f1,4,6`, not a
        CSV parser.  Positionless.  quote= as for field_spans: the fields' contents, their doubled quotes kept."""
        import torch
        self._column_arguments(fields, first, count, delimiter, newline, quote)    # refused before the GPU is touched
        dev = self._device_index()
        n, totals = self._field_columns(fields, first, count, delimiter, newline, quote)
        out = []
        for column, total in enumerate(totals):
            data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
            offsets = torch.empty(n + 1, dtype=torch.int64, device=f"cuda:{dev}")
            sizes = torch.empty(n, dtype=torch.int64, device=f"cuda:{dev}")
            # the new tensors' memory may still be in use by work queued on torch's stream: the copies come after it
            torch.cuda.current_stream(data.device).synchronize()
            self._check(N.lib().mi355x_bz2_reader_take_field_column(
                self._h, column, ctypes.c_void_p(data.data_ptr()) if total else None, ctypes.c_void_p(offsets.data_ptr()),
                ctypes.c_void_p(sizes.data_ptr()) if n else None, 1))
            out.append((data, offsets, sizes))
        return out

    def read_columns(self, fields, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """read_columns_to_tensor on the host -> a list with, per entry of `fields`, a list with one bytes object per line
        and None where the line has no such field: [read_fields(j, ...) for j in fields], from one decode."""
        import numpy as np
        n, totals = self._field_columns(fields, first, count, delimiter, newline, quote)
        out = []
        for column, total in enumerate(totals):
            data = bytearray(total)
            offsets = np.empty(n + 1, dtype=np.uint64)
            sizes = np.empty(n, dtype=np.int64)
            self._check(N.lib().mi355x_bz2_reader_take_field_column(
                self._h, column, (ctypes.c_char * total).from_buffer(data) if total else None, ctypes.c_void_p(offsets.ctypes.data),
                ctypes.c_void_p(sizes.ctypes.data) if n else None, 0))
            data = bytes(data)
            bounds = offsets.tolist()
            out.append([data[bounds[i]:bounds[i + 1]] if size >= 0 else None for i, size in enumerate(sizes.tolist())])
        return out

    # -- field hashes and groups: the KEY of a line is N.line_hash(content.split(delimiter)[field], seed), computed where the
    # decoded bytes lie; a line with fewer fields has the key N.FIELD_MISSING = 2^61 - 1, which no hash takes, and an
    # empty field is present and hashes to 0.  "Distinct value" below means "of distinct key", with the collision bound
    # of line_hashes; a second seed is an independent check.  No quoting, no escaping: `cut -f`, not a CSV parser
    def _field_hash_arguments(self, field, first, count, delimiter, newline, seed):
        nl, dl, field, first, count = self._field_arguments(field, first, count, delimiter, newline)
        (seed,), _ = self._u64([seed], "seed")
        return nl, dl, field, first, count, seed

    def _field_hashes(self, field, first, count, delimiter, newline, seed, tensors):
        nl, dl, field, first, count, seed = self._field_hash_arguments(field, first, count, delimiter, newline, seed)
        L = N.lib()
        return self._columns(lambda keep, n: L.mi355x_bz2_reader_field_hashes(self._h, nl, dl, field, seed, first, count, keep, n),
                             lambda *to: L.mi355x_bz2_reader_take_field_hashes(self._h, *to), ("uint64",), tensors)[0]

    def field_hashes(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """The keys of lines [first, first + count) (count None: to the last line; clipped there) -> numpy uint64, one
        per line: line_hash(content.split(delimiter)[field], seed), or FIELD_MISSING where the line has no such field.
        Only the blocks that hold those lines are decoded, each once; field and hash are found on the GPU in shared
        passes and 8 bytes per line come back.  Builds the line index first if the reader does not hold one for
        `newline`.  Not a CSV parser.  Positionless."""
        return self._field_hashes(field, first, count, delimiter, newline, seed, False)

    def field_hashes_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """field_hashes as a torch.int64 tensor on the reader's device; the keys never pass through the host.  A key is
        below 2^61 and FIELD_MISSING is 2^61 - 1, so torch.unique, sort and isin order and compare them as they are:
        join keys for torch.isin."""
        return self._field_hashes(field, first, count, delimiter, newline, seed, True)

    def _field_groups(self, field, first, count, delimiter, newline, seed):
        """mi355x_bz2_reader_field_groups and its take -> (lines, counts, starts, sizes, missing)."""
        import numpy as np
        nl, dl, field, first, count, seed = self._field_hash_arguments(field, first, count, delimiter, newline, seed)
        n, missing = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_field_groups(self._h, nl, dl, field, seed, first, count, ctypes.byref(n),
                                                            ctypes.byref(missing)))
        lines, counts, starts = (np.empty(n.value, dtype=np.uint64) for _ in range(3))
        sizes = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._check(N.lib().mi355x_bz2_reader_take_field_groups(self._h, lines.ctypes.data, counts.ctypes.data,
                                                                     starts.ctypes.data, sizes.ctypes.data, n.value))
        return lines, counts, starts, sizes, missing.value

    def count_by_field(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """Lines [first, first + count) grouped by field `field` (`cut -f | sort | uniq -c`) -> (lines, counts, missing):
        `lines` (numpy uint64, ascending) holds the file's line number of the first line of every distinct value,
        `counts` (numpy uint64) how many lines of the range have that value, `missing` the number of lines without such a
        field: counts.sum() + missing is the number of lines in the range.  field_hashes, then a sort of the keys on the
        GPU; 32 bytes per distinct value come back and nothing per line.  Not a CSV parser.  Positionless."""
        lines, counts, _, _, missing = self._field_groups(field, first, count, delimiter, newline, seed)
        return lines, counts, missing

    def value_counts(self, field, limit=None, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """count_by_field with the values themselves (`cut -f | sort | uniq -c | sort -rn | head`) -> a list of (value
        bytes, count) by descending count, then by first occurrence, at most `limit` entries (None: all).  The values
        are fetched by read_ranges over the chosen groups' spans, so only those bytes leave the GPU.  Lines without the
        field are in no entry.  Not a CSV parser.  Positionless."""
        import numpy as np
        limit = self._line_limit(limit)
        _, counts, starts, sizes, _ = self._field_groups(field, first, count, delimiter, newline, seed)
        # the groups ascend by first line: a stable sort by descending count keeps that order among equal counts
        chosen = np.argsort(-counts.astype(np.int64), kind="stable")[:limit]
        if len(chosen) == 0:
            return []
        values = self.read_ranges([(int(starts[i]), int(sizes[i])) for i in chosen])
        return [(value, int(counts[i])) for value, i in zip(values, chosen)]

    # -- field numbers and sums: the NUMBER of a line is N.parse_field_number(content.split(delimiter)[field]): the bytes
    # must match [+-]?[0-9]{1,18} from end to end -- no whitespace, no '_', no hex, no floats, at most 18 digits, which
    # always fit int64: this is not awk's strtod and not Python's int().  A present field that is no number gives
    # N.FIELD_NOT_A_NUMBER = -2^63, a line with fewer fields N.FIELD_NUMBER_MISSING = -2^63 + 1; no number takes either.
    # No quoting, no escaping: `cut -f`, not a CSV parser
    def _field_ints(self, field, first, count, delimiter, newline, tensors):
        nl, dl, field, first, count = self._field_arguments(field, first, count, delimiter, newline)
        L = N.lib()
        return self._columns(lambda keep, n: L.mi355x_bz2_reader_field_numbers(self._h, nl, dl, field, first, count, keep, n),
                             lambda *to: L.mi355x_bz2_reader_take_field_numbers(self._h, *to), ("int64",), tensors)[0]

    def field_ints(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n"):
        """Field `field` of lines [first, first + count) (count None: to the last line; clipped there) as numbers ->
        numpy int64, one per line: parse_field_number(content.split(delimiter)[field]) where that is a number
        ([+-]?[0-9]{1,18}: not awk's strtod), FIELD_NOT_A_NUMBER where the field is something else, FIELD_NUMBER_MISSING
        where the line has no such field.  Only the blocks that hold those lines are decoded, each once; the fields are
        found and parsed on the GPU and 8 bytes per line come back.  Builds the line index first if the reader does not
        hold one for `newline`.  Not a CSV parser.  Positionless."""
        return self._field_ints(field, first, count, delimiter, newline, False)

    def field_ints_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n"):
        """field_ints as a torch.int64 tensor on the reader's device; the numbers never pass through the host.  Mask
        the two sentinels (both below -2^63 + 2) before arithmetic."""
        return self._field_ints(field, first, count, delimiter, newline, True)

    # -- rows by a column: the lines whose field `field` is one of a set of values, or whose number lies in a range (`awk
    # -F'\t' '$3 == "GET"'`, `awk '$5 >= 500 && $5 < 600'`, a semi-join on a key column).  A line matches `values` iff it has
    # the field and content.split(delimiter)[field] is byte for byte one of them: the empty value matches an empty field
    # that is present, never a missing one.  It matches between=(lo, hi) iff N.parse_field_number(field) is a number n with
    # lo <= n <= hi; None is an open side; a field that is no number and a missing one never match.  invert=True selects
    # the complement within the line range (`grep -v`).  The key under `seed` only filters in front of the comparison of
    # the bytes: the answer does not depend on it.  It matches regex=pattern (keyword only; bytes-like, or compiled by
    # compile_regex) iff it has the field and the pattern's table, run over the field's bytes, matches: the field is to the
    # pattern what a line's content is to grep_regex, so `^` and `$` anchor to the field's ends (`awk '$3 ~ /^GET$/'`), an
    # empty field that is present matches iff the pattern matches the empty string, a missing field never matches, and a
    # field may have any size.  For a field without the byte 0x0A that is re.search(pattern, field, re.DOTALL), with
    # ignore_case=True re.IGNORECASE too; Python's `$` also matches in front of a trailing b"\n", the table's does not.
    # `seed` is ignored with regex.  No quoting, no escaping: not a CSV parser
    def _where_arguments(self, field, values, between, invert, first, count, limit, delimiter, newline, seed, regex=None,
                         ignore_case=False):
        if regex is None:
            if ignore_case:
                raise ValueError("ignore_case needs regex")
            if (values is None) == (between is None):
                raise ValueError("exactly one of values and between must be given")
        elif values is not None or between is not None:
            raise ValueError("exactly one of values, between and regex must be given")
        nl, dl, field, first, count, seed = self._field_hash_arguments(field, first, count, delimiter, newline, seed)
        if regex is not None:
            predicate = (self._regex(regex, ignore_case),)      # a ValueError for a pattern outside the syntax
        else:
            predicate = N.value_set(values) if values is not None else N.number_range(between)
        return nl, dl, field, first, count, seed, predicate, 1 if invert else 0, self._line_limit(limit)

    def _where_field(self, arguments, limit, keep):
        """mi355x_bz2_reader_field_matches, _field_in_range or _field_matches_regex -> (the numbers held, the lines that
        match)."""
        nl, dl, field, first, count, seed, predicate, invert, _ = arguments
        held, matching = ctypes.c_uint64(), ctypes.c_uint64()
        if len(predicate) == 1:
            self._check(N.lib().mi355x_bz2_reader_field_matches_regex(self._h, nl, dl, field, predicate[0]._h, invert, first, count,
                                                                       limit, keep, ctypes.byref(held), ctypes.byref(matching)))
        elif len(predicate) == 3:
            data, sizes, k = predicate
            self._check(N.lib().mi355x_bz2_reader_field_matches(self._h, nl, dl, field, data, sizes, k, seed, invert, first, count, limit,
                                                                 keep, ctypes.byref(held), ctypes.byref(matching)))
        else:
            self._check(N.lib().mi355x_bz2_reader_field_in_range(self._h, nl, dl, field, *predicate, invert, first, count, limit, keep,
                                                                  ctypes.byref(held), ctypes.byref(matching)))
        return held.value, matching.value

    def where_field(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None, delimiter=b"\t",
                    newline=b"\n", seed=0, *,
                    regex=None, ignore_case=False):
        """The numbers of the lines of [first, first + count) whose field `field` is one of `values` (1 to 1 024 bytes
        objects of 0 to 256 bytes, at most 16 384 bytes in total) or whose number lies in between=(lo, hi) -> numpy uint64,
        ascending, numbered in the file, at most `limit` of them (None: all).  The
        numbers index the arrays of read_columns, field_ints and field_hashes over the same line range (less `first`).
        Every needed block is decoded once; the predicate is evaluated and its flags are compacted on the GPU, and 8 bytes
        per selected line come back.  Two different values with the same key under `seed` are refused: pass another seed.
        Or, keyword only, regex=pattern (bytes-like, or compiled by compile_regex; ignore_case=True folds ASCII letters):
        the lines whose field matches it, `awk -F'\\t' '$7 ~ /^\\/api\\//'`.  The field is to the pattern what the line's
        content is to grep_regex: `^` and `$` anchor to the field's ends, a field of any size is walked, a missing field
        never matches, an empty one matches iff the pattern matches the empty string.  For a field without b"\\n" that is
        re.search(pattern, field, re.DOTALL); Python's `$` also matches in front of a trailing b"\\n", this one does not.
        The syntax and the refusals (a ValueError before anything is launched) are compile_regex's; a GPU lane stops at
        the first byte after which the answer is known, so an anchored prefix costs a few bytes per line.  Exactly one of
        values, between and regex; `seed` is ignored with regex.  Not a CSV parser.  Positionless."""
        import numpy as np
        arguments = self._where_arguments(field, values, between, invert, first, count, limit, delimiter, newline, seed, regex, ignore_case)
        n, _ = self._where_field(arguments, arguments[-1], 0)
        out = np.empty(n, dtype=np.uint64)
        if n:
            self._check(N.lib().mi355x_bz2_reader_take_field_matches(self._h, out.ctypes.data, n, 0))
        return out

    def where_field_to_tensor(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                              delimiter=b"\t", newline=b"\n", seed=0, *,
                              regex=None, ignore_case=False):
        """where_field as a torch.int64 tensor on the reader's device; the numbers never pass through the host.  Less
        `first`, it indexes the tensors of read_columns_to_tensor, field_ints_to_tensor and field_hashes_to_tensor."""
        import torch
        arguments = self._where_arguments(field, values, between, invert, first, count, limit, delimiter, newline, seed, regex, ignore_case)
        dev = self._device_index()
        n, _ = self._where_field(arguments, arguments[-1], 1)
        out = torch.empty(n, dtype=torch.int64, device=f"cuda:{dev}")
        if n:
            torch.cuda.current_stream(out.device).synchronize()
            self._check(N.lib().mi355x_bz2_reader_take_field_matches(self._h, ctypes.c_void_p(out.data_ptr()), n, 1))
        return out

    def count_where_field(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                          delimiter=b"\t", newline=b"\n", seed=0, *,
                          regex=None, ignore_case=False):
        """len(where_field(...)) without the numbers: nothing per line leaves the GPU, 8 bytes come back."""
        arguments = self._where_arguments(field, values, between, invert, first, count, limit, delimiter, newline, seed, regex, ignore_case)
        _, matching = self._where_field(arguments, 0, 0)
        return min(matching, arguments[-1])

    def _select_lines(self, arguments, on_device):
        """mi355x_bz2_reader_select_lines and the numbers and sizes of the held lines (_take_grep), as _grep."""
        import numpy as np
        nl, dl, field, first, count, seed, predicate, invert, limit = arguments
        if limit == 0:
            return np.empty(0, dtype=np.uint64), [], 0
        n, total = ctypes.c_uint64(), ctypes.c_uint64()
        if len(predicate) == 1:
            self._check(N.lib().mi355x_bz2_reader_select_lines_regex(self._h, nl, dl, field, predicate[0]._h, invert, first, count,
                                                                      limit, 1 if on_device else 0, ctypes.byref(n),
                                                                      ctypes.byref(total)))
        else:
            if len(predicate) == 3:
                data, sizes, k = predicate
                bounds = (0, 0, 0, 0)
            else:
                data, sizes, k, bounds = None, None, 0, predicate
            self._check(N.lib().mi355x_bz2_reader_select_lines(self._h, nl, dl, field, data, sizes, k, seed, *bounds, invert, first,
                                                                count, limit, 1 if on_device else 0, ctypes.byref(n),
                                                                ctypes.byref(total)))
        numbers = (ctypes.c_uint64 * max(1, n.value))()
        sizes = (ctypes.c_uint64 * max(1, n.value))()
        self._check(N.lib().mi355x_bz2_reader_take_grep(self._h, numbers, sizes, n.value))
        return (np.frombuffer(numbers, dtype=np.uint64, count=n.value).copy(), [sizes[i] for i in range(n.value)], total.value)

    def select_lines(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None, delimiter=b"\t",
                     newline=b"\n", seed=0, *,
                     regex=None, ignore_case=False):
        """The lines where_field selects -> (numbers, lines) as grep returns them: the line numbers (numpy uint64,
        ascending) and one bytes object per line, whole and with its delimiter, at most `limit` lines (None: all).  The
        selection, then the lines themselves in a second pass over the blocks that hold them.  Releases line ranges held
        by earlier calls.  Positionless."""
        arguments = self._where_arguments(field, values, between, invert, first, count, limit, delimiter, newline, seed, regex, ignore_case)
        numbers, sizes, total = self._select_lines(arguments, False)
        if arguments[-1] == 0:
            return numbers, []
        out = bytearray(total)
        dst = (ctypes.c_char * max(1, total)).from_buffer(out) if total > 0 else None
        self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, dst, 0))
        del dst
        lines, at = [], 0
        for size in sizes:
            lines.append(bytes(out[at:at + size]))
            at += size
        return numbers, lines

    def select_lines_to_tensor(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                               delimiter=b"\t", newline=b"\n", seed=0, *,
                               regex=None, ignore_case=False):
        """select_lines into ONE contiguous torch.uint8 tensor on the reader's device -> (numbers, data, offsets) as
        grep_to_tensor returns them: line i is ``data[offsets[i]:offsets[i + 1]]``."""
        import torch
        arguments = self._where_arguments(field, values, between, invert, first, count, limit, delimiter, newline, seed, regex, ignore_case)
        dev = self._device_index()
        numbers, sizes, total = self._select_lines(arguments, True)
        data = torch.empty(total, dtype=torch.uint8, device=f"cuda:{dev}")
        if total:
            torch.cuda.current_stream(data.device).synchronize()
        if arguments[-1] != 0:
            self._check(N.lib().mi355x_bz2_reader_take_line_ranges(self._h, ctypes.c_void_p(data.data_ptr()) if total else None, 1))
        bounds = [0]
        for size in sizes:
            bounds.append(bounds[-1] + size)
        return numbers, data, torch.tensor(bounds, dtype=torch.int64)

    def _field_sums(self, key_field, value_field, first, count, delimiter, newline, seed):
        """mi355x_bz2_reader_field_sums and its take -> (lines, counts, starts, sizes, numbers, sums, mins, maxs, missing)."""
        import numpy as np
        nl, dl, key_field, first, count, seed = self._field_hash_arguments(key_field, first, count, delimiter, newline, seed)
        value_field = self._field_arguments(value_field, first, count, delimiter, newline)[2]
        n, missing = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(N.lib().mi355x_bz2_reader_field_sums(self._h, nl, dl, key_field, value_field, seed, first, count,
                                                          ctypes.byref(n), ctypes.byref(missing)))
        lines, counts, starts, numbers, lo = (np.empty(n.value, dtype=np.uint64) for _ in range(5))
        sizes, hi, mins, maxs = (np.empty(n.value, dtype=np.int64) for _ in range(4))
        if n.value:
            self._check(N.lib().mi355x_bz2_reader_take_field_sums(
                self._h, *[a.ctypes.data for a in (lines, counts, starts, sizes, numbers, lo, hi, mins, maxs)], n.value))
        sums = [(int(h) << 64) + int(l) for h, l in zip(hi, lo)]
        return lines, counts, starts, sizes, numbers, sums, mins, maxs, missing.value

    def sum_by_field(self, key_field, value_field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """Lines [first, first + count) grouped by field `key_field`, with field `value_field` summed per group
        (`awk -F'\\t' '{s[$1]+=$3}'`, but exact and with parse_field_number's numbers: not awk's strtod) -> (lines,
        counts, numbers, sums, mins, maxs, missing).  `lines` (numpy uint64, ascending) holds the file's line number of
        the first line of every distinct key, `counts` (numpy uint64) how many lines of the range have that key,
        `numbers` (numpy uint64) how many of those have a number in the value field, `sums` (a list of Python ints) their
        exact sum, `mins` and `maxs` (numpy int64) the least and the largest of them, FIELD_NOT_A_NUMBER where `numbers`
        is 0, and `missing` the number of lines without the key field.  Every needed block is decoded once: keys and
        numbers are found on the GPU over the same resident bytes, sorted and reduced there; 72 bytes per distinct key come
        back and nothing per line.  key_field == value_field is allowed.  Not a CSV parser.  Positionless."""
        lines, counts, _, _, numbers, sums, mins, maxs, missing = self._field_sums(key_field, value_field, first, count, delimiter,
                                                                                   newline, seed)
        return lines, counts, numbers, sums, mins, maxs, missing

    def value_sums(self, key_field, value_field, limit=None, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """sum_by_field with the keys themselves -> a list of (key bytes, sum, numbers) by descending sum, then by first
        occurrence, at most `limit` entries (None: all).  The keys are fetched by read_ranges over the chosen groups'
        spans, so only those bytes leave the GPU.  Lines without the key field are in no entry.  Numbers are
        parse_field_number's (not awk's strtod).  Not a CSV parser.  Positionless."""
        limit = self._line_limit(limit)
        _, _, starts, sizes, numbers, sums, _, _, _ = self._field_sums(key_field, value_field, first, count, delimiter, newline, seed)
        # the groups ascend by first line: a stable sort by descending sum keeps that order among equal sums
        chosen = sorted(range(len(sums)), key=lambda i: -sums[i])[:limit]
        if len(chosen) == 0:
            return []
        values = self.read_ranges([(int(starts[i]), int(sizes[i])) for i in chosen])
        return [(value, sums[i], int(numbers[i])) for value, i in zip(values, chosen)]

    # -- a set of patterns: a match is a pair (p, i) with data[p:p + len(patterns[i])] == patterns[i], start <= p and
    # p + len(patterns[i]) <= end; a result is ordered by p, then i.  Every block of the range is decoded once per call.
    # With ignore_case=True both sides are compared under bytes.lower(); patterns that are then equal, or prefixes of one
    # another, still report their own pairs
    def _search_set(self, patterns, start, end, limit, ignore_case=False):
        """Step 1 (mi355x_bz2_reader_search_set_ex): (number of pairs, or of the pairs now held; per-pattern counts, which
        the native call fills for limit 0 only)."""
        import numpy as np
        self._require()
        data, sizes, k = N.pattern_set(patterns)
        start, end = int(start), 2**64 - 1 if end is None else int(end)
        if start < 0 or end < 0:
            raise ValueError("start and end must not be negative")
        n = ctypes.c_uint64()
        each = np.zeros(k, dtype=np.uint64)
        self._check(N.lib().mi355x_bz2_reader_search_set_ex(self._h, data, sizes, k, self._flags(ignore_case),
                                                            min(start, 2**64 - 1), min(end, 2**64 - 1), limit, ctypes.byref(n),
                                                            each.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return n.value, each

    def count_matches_each(self, patterns, start=0, end=None, *, ignore_case=False):
        """How often each byte string of the sequence `patterns` (1 to 1 024 of them, 1 to 256 bytes each, at most 16 384
        bytes in total) occurs in data[start:end] -> numpy uint64, one count per pattern in the caller's order, each
        equal to count_matches of that pattern.  Equal patterns and prefixes of one another are allowed.  ONE decode of
        every block of the range whatever the number of patterns; only the counts leave the GPU.  Positionless."""
        return self._search_set(patterns, start, end, 0, ignore_case)[1]

    def find_all_any(self, patterns, start=0, end=None, limit=None, *, ignore_case=False):
        """The occurrences of every pattern of `patterns` in data[start:end] -> (positions numpy uint64, ids numpy
        uint32): pairs (offset, index of the pattern that occurs there) by ascending offset, then ascending index, at
        most `limit` of them (None: all).  The pairs of pattern i are exactly find_all(patterns[i], start, end), and the
        result with a limit is the first `limit` pairs of the result without one.  Positionless."""
        import numpy as np
        if limit is not None and int(limit) < 0:
            raise ValueError("limit must not be negative")
        if limit is not None and int(limit) == 0:
            N.pattern_set(patterns)
            return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint32)
        n, _ = self._search_set(patterns, start, end, 2**64 - 1 if limit is None else min(int(limit), 2**64 - 1), ignore_case)
        positions, ids = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint32)
        self._check(N.lib().mi355x_bz2_reader_take_set_matches(
            self._h, positions.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if n else None,
            ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if n else None, n))
        return positions, ids

    def find_any(self, patterns, start=0, end=None, *, ignore_case=False):
        """(offset, index) of the first occurrence of any pattern of `patterns` in data[start:end] -- the lowest index
        among those that occur at that offset --, or (-1, -1): find_all_any with limit=1."""
        positions, ids = self.find_all_any(patterns, start, end, 1, ignore_case=ignore_case)
        return (int(positions[0]), int(ids[0])) if len(positions) else (-1, -1)

    def grep_any(self, patterns, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """grep for a set of patterns (`grep -n -F -f FILE`) -> (numbers, lines): the lines that hold the first byte of an
        occurrence of at least one pattern, each once.  The set search is the first pass (one decode of the range
        whatever the number of patterns); the rank and line passes are grep's."""
        return self._grep_lines(patterns, start, end, limit, newline, True, ignore_case)

    def count_matching_lines_any(self, patterns, start=0, end=None, newline=b"\n", *, ignore_case=False):
        """The number of distinct lines that hold an occurrence of at least one pattern (`grep -c -F -f FILE`)."""
        return self._grep(patterns, start, end, 0, newline, False, True, ignore_case)

    def grep_any_to_tensor(self, patterns, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """grep_any into ONE contiguous torch.uint8 tensor on the reader's device -> (numbers, data, offsets), as
        grep_to_tensor."""
        return self._grep_tensor(patterns, start, end, limit, newline, True, ignore_case)

    def set_verify_stream_crc(self, enable: bool):
        """Check every end-of-stream CRC against the block CRCs in front of it (default: only with parallelization=1,
        like the reference, whose serial reader checks and whose parallel reader does not)."""
        self._require()
        self._check(N.lib().mi355x_bz2_reader_set_verify_stream_crc(self._h, 1 if enable else 0))

    def streams_verified(self) -> int:
        self._require()
        return int(N.lib().mi355x_bz2_reader_streams_verified(self._h))

    def statistics(self):
        self._require()
        st = N.ReaderStats()
        self._check(N.lib().mi355x_bz2_reader_statistics(self._h, ctypes.byref(st)))
        return st.as_dict()


class IndexedBzip2FileRaw(io.RawIOBase):
    """indexed_bzip2.pyx:290-317"""

    def __init__(self, filename, parallelization=1, device=-1):
        self.bz2reader = _IndexedBzip2FileParallel(filename, parallelization, device)
        self.name = filename
        self.mode = "rb"

        self.readinto = self.bz2reader.readinto
        self.seek = self.bz2reader.seek
        self.tell = self.bz2reader.tell
        self.seekable = self.bz2reader.seekable
        self.join_threads = self.bz2reader.join_threads

    def close(self):
        if self.closed:
            return
        super().close()
        self.bz2reader.close()

    def readable(self):
        return True


class IndexedBzip2File(io.BufferedReader):
    """indexed_bzip2.pyx:320-337"""

    def __init__(self, filename, parallelization=1, device=-1):
        fobj = IndexedBzip2FileRaw(filename, parallelization, device)
        self.bz2reader = fobj.bz2reader

        self.tell_compressed = self.bz2reader.tell_compressed
        self.block_offsets = self.bz2reader.block_offsets
        self.set_block_offsets = self.bz2reader.set_block_offsets
        self.block_offsets_complete = self.bz2reader.block_offsets_complete
        self.available_block_offsets = self.bz2reader.available_block_offsets
        self.size = self.bz2reader.size
        self.join_threads = self.bz2reader.join_threads
        self.statistics = self.bz2reader.statistics
        self.set_verify_stream_crc = self.bz2reader.set_verify_stream_crc
        self.streams_verified = self.bz2reader.streams_verified

        super().__init__(fobj, buffer_size=1024**2)

    # positionless: the buffered reader's position and read-ahead stay valid
    def read_ranges(self, ranges):
        """See _IndexedBzip2FileParallel.read_ranges."""
        if self.closed:
            raise ValueError("I/O operation on closed file.")
        return self.bz2reader.read_ranges(ranges)

    def read_ranges_into(self, offsets, sizes, out):
        """See _IndexedBzip2FileParallel.read_ranges_into."""
        if self.closed:
            raise ValueError("I/O operation on closed file.")
        return self.bz2reader.read_ranges_into(offsets, sizes, out)

    def _open_reader(self):
        if self.closed:
            raise ValueError("I/O operation on closed file.")
        return self.bz2reader

    def line_offsets(self, newline=b"\n"):
        """See _IndexedBzip2FileParallel.line_offsets."""
        return self._open_reader().line_offsets(newline)

    def set_line_offsets(self, offsets, newline=b"\n"):
        """See _IndexedBzip2FileParallel.set_line_offsets."""
        return self._open_reader().set_line_offsets(offsets, newline)

    def count_lines(self, newline=b"\n"):
        """See _IndexedBzip2FileParallel.count_lines."""
        return self._open_reader().count_lines(newline)

    def line_starts(self, lines, newline=b"\n"):
        """See _IndexedBzip2FileParallel.line_starts."""
        return self._open_reader().line_starts(lines, newline)

    def read_line_ranges(self, ranges, newline=b"\n"):
        """See _IndexedBzip2FileParallel.read_line_ranges."""
        return self._open_reader().read_line_ranges(ranges, newline)

    def read_lines(self, first, count=1, newline=b"\n"):
        """See _IndexedBzip2FileParallel.read_lines."""
        return self._open_reader().read_lines(first, count, newline)

    def read_line_ranges_to_tensor(self, ranges, newline=b"\n"):
        """See _IndexedBzip2FileParallel.read_line_ranges_to_tensor."""
        return self._open_reader().read_line_ranges_to_tensor(ranges, newline)

    def count_matches(self, pattern, start=0, end=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_matches."""
        return self._open_reader().count_matches(pattern, start, end, ignore_case=ignore_case)

    def find_all(self, pattern, start=0, end=None, limit=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.find_all."""
        return self._open_reader().find_all(pattern, start, end, limit, ignore_case=ignore_case)

    def find(self, pattern, start=0, end=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.find."""
        return self._open_reader().find(pattern, start, end, ignore_case=ignore_case)

    def line_numbers(self, offsets, newline=b"\n"):
        """See _IndexedBzip2FileParallel.line_numbers."""
        return self._open_reader().line_numbers(offsets, newline)

    def grep(self, pattern, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep."""
        return self._open_reader().grep(pattern, start, end, limit, newline, ignore_case=ignore_case)

    def count_matching_lines(self, pattern, start=0, end=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_matching_lines."""
        return self._open_reader().count_matching_lines(pattern, start, end, newline, ignore_case=ignore_case)

    def grep_to_tensor(self, pattern, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep_to_tensor."""
        return self._open_reader().grep_to_tensor(pattern, start, end, limit, newline, ignore_case=ignore_case)

    def grep_regex(self, pattern, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep_regex."""
        return self._open_reader().grep_regex(pattern, limit, newline, ignore_case=ignore_case)

    def count_matching_lines_regex(self, pattern, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_matching_lines_regex."""
        return self._open_reader().count_matching_lines_regex(pattern, newline, ignore_case=ignore_case)

    def grep_regex_to_tensor(self, pattern, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep_regex_to_tensor."""
        return self._open_reader().grep_regex_to_tensor(pattern, limit, newline, ignore_case=ignore_case)

    def line_hashes(self, first=0, count=None, newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.line_hashes."""
        return self._open_reader().line_hashes(first, count, newline, seed)

    def line_hashes_to_tensor(self, first=0, count=None, newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.line_hashes_to_tensor."""
        return self._open_reader().line_hashes_to_tensor(first, count, newline, seed)

    def count_distinct_lines(self, newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.count_distinct_lines."""
        return self._open_reader().count_distinct_lines(newline, seed)

    def first_occurrences(self, newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.first_occurrences."""
        return self._open_reader().first_occurrences(newline, seed)

    def field_spans(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.field_spans."""
        return self._open_reader().field_spans(field, first, count, delimiter, newline, quote=quote)

    def field_spans_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.field_spans_to_tensor."""
        return self._open_reader().field_spans_to_tensor(field, first, count, delimiter, newline, quote=quote)

    def field_hashes(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.field_hashes."""
        return self._open_reader().field_hashes(field, first, count, delimiter, newline, seed)

    def field_hashes_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.field_hashes_to_tensor."""
        return self._open_reader().field_hashes_to_tensor(field, first, count, delimiter, newline, seed)

    def count_by_field(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.count_by_field."""
        return self._open_reader().count_by_field(field, first, count, delimiter, newline, seed)

    def value_counts(self, field, limit=None, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.value_counts."""
        return self._open_reader().value_counts(field, limit, first, count, delimiter, newline, seed)

    def field_ints(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n"):
        """See _IndexedBzip2FileParallel.field_ints."""
        return self._open_reader().field_ints(field, first, count, delimiter, newline)

    def field_ints_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n"):
        """See _IndexedBzip2FileParallel.field_ints_to_tensor."""
        return self._open_reader().field_ints_to_tensor(field, first, count, delimiter, newline)

    def where_field(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None, delimiter=b"\t",
                    newline=b"\n", seed=0, *,
                    regex=None, ignore_case=False):
        """See _IndexedBzip2FileParallel.where_field."""
        return self._open_reader().where_field(field, values, between, invert, first, count, limit, delimiter, newline, seed,
                                              regex=regex, ignore_case=ignore_case)

    def where_field_to_tensor(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                              delimiter=b"\t", newline=b"\n", seed=0, *,
                              regex=None, ignore_case=False):
        """See _IndexedBzip2FileParallel.where_field_to_tensor."""
        return self._open_reader().where_field_to_tensor(field, values, between, invert, first, count, limit, delimiter, newline, seed,
                                                        regex=regex, ignore_case=ignore_case)

    def count_where_field(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                          delimiter=b"\t", newline=b"\n", seed=0, *,
                          regex=None, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_where_field."""
        return self._open_reader().count_where_field(field, values, between, invert, first, count, limit, delimiter, newline, seed,
                                                    regex=regex, ignore_case=ignore_case)

    def select_lines(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None, delimiter=b"\t",
                     newline=b"\n", seed=0, *,
                     regex=None, ignore_case=False):
        """See _IndexedBzip2FileParallel.select_lines."""
        return self._open_reader().select_lines(field, values, between, invert, first, count, limit, delimiter, newline, seed,
                                               regex=regex, ignore_case=ignore_case)

    def select_lines_to_tensor(self, field, values=None, between=None, invert=False, first=0, count=None, limit=None,
                               delimiter=b"\t", newline=b"\n", seed=0, *,
                               regex=None, ignore_case=False):
        """See _IndexedBzip2FileParallel.select_lines_to_tensor."""
        return self._open_reader().select_lines_to_tensor(field, values, between, invert, first, count, limit, delimiter, newline, seed,
                                                         regex=regex, ignore_case=ignore_case)

    def sum_by_field(self, key_field, value_field, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.sum_by_field."""
        return self._open_reader().sum_by_field(key_field, value_field, first, count, delimiter, newline, seed)

    def value_sums(self, key_field, value_field, limit=None, first=0, count=None, delimiter=b"\t", newline=b"\n", seed=0):
        """See _IndexedBzip2FileParallel.value_sums."""
        return self._open_reader().value_sums(key_field, value_field, limit, first, count, delimiter, newline, seed)

    def read_fields(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.read_fields."""
        return self._open_reader().read_fields(field, first, count, delimiter, newline, quote=quote)

    def read_fields_to_tensor(self, field, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.read_fields_to_tensor."""
        return self._open_reader().read_fields_to_tensor(field, first, count, delimiter, newline, quote=quote)

    def read_columns(self, fields, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.read_columns."""
        return self._open_reader().read_columns(fields, first, count, delimiter, newline, quote=quote)

    def read_columns_to_tensor(self, fields, first=0, count=None, delimiter=b"\t", newline=b"\n", *, quote=None):
        """See _IndexedBzip2FileParallel.read_columns_to_tensor."""
        return self._open_reader().read_columns_to_tensor(fields, first, count, delimiter, newline, quote=quote)

    def count_matches_each(self, patterns, start=0, end=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_matches_each."""
        return self._open_reader().count_matches_each(patterns, start, end, ignore_case=ignore_case)

    def find_all_any(self, patterns, start=0, end=None, limit=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.find_all_any."""
        return self._open_reader().find_all_any(patterns, start, end, limit, ignore_case=ignore_case)

    def find_any(self, patterns, start=0, end=None, *, ignore_case=False):
        """See _IndexedBzip2FileParallel.find_any."""
        return self._open_reader().find_any(patterns, start, end, ignore_case=ignore_case)

    def grep_any(self, patterns, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep_any."""
        return self._open_reader().grep_any(patterns, start, end, limit, newline, ignore_case=ignore_case)

    def count_matching_lines_any(self, patterns, start=0, end=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.count_matching_lines_any."""
        return self._open_reader().count_matching_lines_any(patterns, start, end, newline, ignore_case=ignore_case)

    def grep_any_to_tensor(self, patterns, start=0, end=None, limit=None, newline=b"\n", *, ignore_case=False):
        """See _IndexedBzip2FileParallel.grep_any_to_tensor."""
        return self._open_reader().grep_any_to_tensor(patterns, start, end, limit, newline, ignore_case=ignore_case)


builtins_open = builtins.open


def open(filename, parallelization=1, device=-1):
    """
    filename: can be a file path, a file descriptor, or a file object
              with suitable read, seekable, seek, and tell methods.          (indexed_bzip2.pyx:340-345)
    parallelization: 1 (default, as in the reference) = block by block with the stream-CRC check of the reference's
              serial reader; 0 = default GPU batch (512 blocks); N = N blocks per GPU batch.
    """
    return IndexedBzip2File(filename, parallelization, device)


def write_block_offsets(offsets, file):
    """Block map as text, one "<compressed bit offset>,<decoded byte offset>" per line: the format `ibzip2 -L` writes
    (src/tools/ibzip2.cpp:83-93) and `ibzip2-mi355x -L` reproduces.  `file` is a path or a text file object."""
    text = "".join(f"{int(bits)},{int(byts)}\n" for bits, byts in sorted(offsets.items()))
    if hasattr(file, "write"):
        file.write(text)
    else:
        with builtins_open(file, "w") as f:
            f.write(text)


def read_block_offsets(file):
    """Inverse of write_block_offsets: returns the dict that set_block_offsets() takes."""
    if hasattr(file, "read"):
        text = file.read()
    else:
        with builtins_open(file, "r") as f:
            text = f.read()
    if isinstance(text, bytes):
        text = text.decode("ascii")
    offsets = {}
    for number, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line:
            continue
        parts = line.split(",")
        if len(parts) != 2:
            raise ValueError(f"line {number}: expected '<compressed bits>,<decoded bytes>', got {line!r}")
        offsets[int(parts[0])] = int(parts[1])
    return offsets


def write_line_offsets(offsets, file):
    """Line index (line_offsets()) as text, one "<decoded byte offset>,<line offset>" per line.  `file` is a path or a
    text file object."""
    text = "".join(f"{int(byts)},{int(lines)}\n" for byts, lines in sorted(offsets.items()))
    if hasattr(file, "write"):
        file.write(text)
    else:
        with builtins_open(file, "w") as f:
            f.write(text)


def read_line_offsets(file):
    """Inverse of write_line_offsets: returns the dict that set_line_offsets() takes."""
    if hasattr(file, "read"):
        text = file.read()
    else:
        with builtins_open(file, "r") as f:
            text = f.read()
    if isinstance(text, bytes):
        text = text.decode("ascii")
    offsets = {}
    for number, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line:
            continue
        parts = line.split(",")
        if len(parts) != 2:
            raise ValueError(f"line {number}: expected '<decoded bytes>,<line offset>', got {line!r}")
        offsets[int(parts[0])] = int(parts[1])
    return offsets
