"""What the reader holds between a step-1 call and its take, walked through the C entry points: which call releases what,
and that the takes of hashes, field spans, field hashes, distinct numbers and field groups do not release ("Held
results").

The input is the `tail` variant of readershapes.py at parallelization 64: a whole-file call is eight launches, and lines
cross their seams (both asserted below).  Every value is compared with readershapes.expected."""
import ctypes

import numpy as np
import pytest

import readershapes as R
from readershapes import NL, TAB

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT = 0, 103
ALL = 2**64 - 1
PARALLELIZATION = 64
COMMA = ord(",")
HELD_BYTES_ROOM = 1 << 16                                       # more than lines 3 and 4 of the corpus hold
UNTOUCHED = 0x5555555555555555                                  # what a take's destination holds before the call


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    e = R.expected("tail")
    path = tmp_path_factory.mktemp("held") / "tail.bz2"
    path.write_bytes(e["enc"])
    return e, str(path)


class Calls:
    """The reader's C entry points for one open reader; a take returns (status, values as lists)."""

    def __init__(self, native, f):
        self.lib, self.f, self.h = native.lib(), f, f._open_reader()._h

    def _step1(self, call, *arguments):
        n = ctypes.c_uint64(7)
        status = call(self.h, *arguments, ctypes.byref(n))
        assert status == OK, self.lib.mi355x_bz2_reader_last_error(self.h)
        return n.value

    def _take(self, call, dtypes, capacity, room=None):
        room = capacity if room is None else room
        columns = [np.full(max(room, 1), UNTOUCHED, dtype=dtype) for dtype in dtypes]
        status = call(self.h, *[c.ctypes.data if capacity else None for c in columns], capacity, 0)
        return status, [c[:room].tolist() for c in columns]

    def hold_line_ranges(self):
        """Lines 3 and 4 held for take_line_ranges -> their bytes."""
        first, count = (ctypes.c_uint64 * 1)(3), (ctypes.c_uint64 * 1)(2)
        sizes, total = (ctypes.c_uint64 * 1)(), ctypes.c_uint64()
        assert self.lib.mi355x_bz2_reader_read_line_ranges(self.h, NL, first, count, 1, 0, sizes, ctypes.byref(total)) == OK
        assert total.value > 0
        return total.value

    def take_line_ranges(self, total):
        """(status, bytes) of a take into a real destination of `total` bytes."""
        destination = ctypes.create_string_buffer(total)
        status = self.lib.mi355x_bz2_reader_take_line_ranges(self.h, destination, 0)
        return status, destination.raw

    def take_line_ranges_is_refused(self):
        """With a real destination, so that only "nothing is held" can refuse the take; the message says so."""
        status, _ = self.take_line_ranges(HELD_BYTES_ROOM)
        return status == INVALID_ARGUMENT and b"no line ranges are held" in self.lib.mi355x_bz2_reader_last_error(self.h)

    def line_hashes(self, first=0, count=ALL, seed=0, keep=0):
        return self._step1(self.lib.mi355x_bz2_reader_line_hashes, NL, seed, first, count, keep)

    def take_line_hashes(self, capacity, room=None):
        status, columns = self._take(self.lib.mi355x_bz2_reader_take_line_hashes, [np.uint64], capacity, room)
        return status, columns[0]

    def line_hashes_device(self):
        return self.lib.mi355x_bz2_reader_line_hashes_device(self.h)

    def field_spans(self, field, dl=TAB, first=0, count=ALL, keep=0):
        return self._step1(self.lib.mi355x_bz2_reader_field_spans, NL, dl, field, first, count, keep)

    def take_field_spans(self, capacity, room=None):
        status, (starts, sizes) = self._take(self.lib.mi355x_bz2_reader_take_field_spans, [np.uint64, np.int64], capacity, room)
        return status, list(zip(starts, sizes))

    def field_hashes(self, field, dl=TAB, seed=0, first=0, count=ALL, keep=0):
        return self._step1(self.lib.mi355x_bz2_reader_field_hashes, NL, dl, field, seed, first, count, keep)

    def take_field_hashes(self, capacity, room=None):
        status, columns = self._take(self.lib.mi355x_bz2_reader_take_field_hashes, [np.uint64], capacity, room)
        return status, columns[0]

    def distinct_lines(self, want_numbers, seed=0):
        return self._step1(self.lib.mi355x_bz2_reader_distinct_lines, NL, seed, want_numbers)

    def take_distinct_lines(self, capacity):
        numbers = (ctypes.c_uint64 * max(capacity, 1))()
        status = self.lib.mi355x_bz2_reader_take_distinct_lines(self.h, numbers if capacity else None, capacity)
        return status, list(numbers[:capacity])

    def field_groups(self, field, dl=TAB, seed=0, first=0, count=ALL):
        n, missing = ctypes.c_uint64(7), ctypes.c_uint64(7)
        status = self.lib.mi355x_bz2_reader_field_groups(self.h, NL, dl, field, seed, first, count, ctypes.byref(n), ctypes.byref(missing))
        assert status == OK, self.lib.mi355x_bz2_reader_last_error(self.h)
        return n.value, missing.value

    def take_field_groups(self, capacity):
        columns = [np.full(max(capacity, 1), UNTOUCHED, dtype=dtype) for dtype in (np.uint64, np.uint64, np.uint64, np.int64)]
        status = self.lib.mi355x_bz2_reader_take_field_groups(self.h, *[c.ctypes.data for c in columns], capacity)
        return status, [c[:capacity].tolist() for c in columns]

    def launches(self):
        return self.f.statistics()["batches"]


def window_on_a_seam(e):
    """(first, count): eight lines around a line that crosses a launch boundary of a whole-file call."""
    raw = e["raw"]
    crossing = [b for b in R.boundaries_of(e["block_starts"], PARALLELIZATION) if raw[b - 1] != NL and raw[b] != NL]
    assert crossing, "no line crosses a seam of this shape"
    return int(np.searchsorted(e["newlines"], crossing[0], "left")) - 3, 8


def test_every_family_keeps_its_own_result(native, corpus, monkeypatch):
    e, path = corpus
    monkeypatch.delenv("MI355X_BZ2_READER_CONTEXTS", raising=False)
    monkeypatch.delenv("MI355X_BZ2_INPUT_BUDGET", raising=False)
    n = len(e["lines"])
    hashes, spans3, keys3 = e["hashes"], e["spans"][(3, TAB)], e["keys"][(3, TAB, 1)]
    first, count = window_on_a_seam(e)
    with native.open(path, parallelization=PARALLELIZATION) as f:
        c = Calls(native, f)
        # nothing was ever held
        assert c.take_line_hashes(4)[0] == INVALID_ARGUMENT and c.take_field_spans(4)[0] == INVALID_ARGUMENT
        assert c.take_field_hashes(4)[0] == INVALID_ARGUMENT and c.take_distinct_lines(4)[0] == INVALID_ARGUMENT
        assert c.take_field_groups(4)[0] == INVALID_ARGUMENT and c.take_line_ranges_is_refused()
        assert c.line_hashes_device() is None

        # held line ranges are served, once: take_line_ranges_is_refused tells held from released
        total = c.hold_line_ranges()
        assert total <= HELD_BYTES_ROOM and not c.take_line_ranges_is_refused()
        total = c.hold_line_ranges()
        ext = e["line_starts"].tolist() + [len(e["raw"])]
        assert c.take_line_ranges(total) == (OK, e["raw"][ext[3]:ext[5]]) and c.take_line_ranges_is_refused()

        # line_hashes: releases the line ranges; the other families still hold nothing
        c.hold_line_ranges()
        before = c.launches()
        assert c.line_hashes() == n
        assert c.launches() - before >= 2, "the whole-file call is one launch: no seam is stitched"
        assert c.take_line_ranges_is_refused()
        assert c.take_line_hashes(n) == (OK, hashes[0]) and c.take_line_hashes(n) == (OK, hashes[0]), "a second take repeats the first"
        assert c.line_hashes_device() is None, "keep_on_device was 0"
        assert c.take_field_spans(4)[0] == INVALID_ARGUMENT and c.take_field_hashes(4)[0] == INVALID_ARGUMENT
        # fewer than are held: the first `capacity`, nothing behind them
        status, some = c.take_line_hashes(5, room=7)
        assert status == OK and some == hashes[0][:5] + [UNTOUCHED] * 2

        # field_spans: releases the line ranges and nothing else
        c.hold_line_ranges()
        assert c.field_spans(3) == n
        assert c.take_line_ranges_is_refused()
        assert c.take_field_spans(n) == (OK, spans3) and c.take_field_spans(n) == (OK, spans3)
        assert c.take_line_hashes(n) == (OK, hashes[0]), "field_spans released the hashes"
        assert c.take_field_hashes(4)[0] == INVALID_ARGUMENT

        # field_hashes: releases the line ranges and nothing of the other two
        c.hold_line_ranges()
        assert c.field_hashes(3, seed=1) == n
        assert c.take_line_ranges_is_refused()
        assert c.take_field_hashes(n) == (OK, keys3) and c.take_field_hashes(n) == (OK, keys3)
        assert c.take_line_hashes(n) == (OK, hashes[0]), "field_hashes released the hashes"
        assert c.take_field_spans(n) == (OK, spans3), "field_hashes released the field spans"
        assert c.take_field_groups(4)[0] == INVALID_ARGUMENT

        # each family again, over a window on a seam: its own result is replaced, the others stay
        assert c.line_hashes(first, count, seed=1) == count
        assert c.take_line_hashes(count) == (OK, hashes[1][first:first + count])
        assert c.take_field_spans(n) == (OK, spans3) and c.take_field_hashes(n) == (OK, keys3)
        assert c.field_spans(1, COMMA, first, count) == count
        assert c.take_field_spans(count) == (OK, e["spans"][(1, COMMA)][first:first + count])
        assert c.take_line_hashes(count) == (OK, hashes[1][first:first + count]) and c.take_field_hashes(n) == (OK, keys3)
        assert c.field_hashes(1, COMMA, 0, first, count) == count
        assert c.take_field_hashes(count) == (OK, e["keys"][(1, COMMA, 0)][first:first + count])
        assert c.take_line_hashes(count) == (OK, hashes[1][first:first + count])
        assert c.take_field_spans(count) == (OK, e["spans"][(1, COMMA)][first:first + count])
        assert f.tell() == 0


def test_distinct_lines_and_field_groups(native, corpus, monkeypatch):
    e, path = corpus
    monkeypatch.delenv("MI355X_BZ2_READER_CONTEXTS", raising=False)
    monkeypatch.delenv("MI355X_BZ2_INPUT_BUDGET", raising=False)
    n = len(e["lines"])
    first, count = window_on_a_seam(e)
    spans = e["spans"][(3, TAB)]
    lines, counts, missing, _ = e["groups"][(3, TAB)]
    window_spans, window_keys = spans[first:first + count], e["keys"][(3, TAB, 0)][first:first + count]
    with native.open(path, parallelization=PARALLELIZATION) as f:
        c = Calls(native, f)
        assert c.field_spans(3, first=first, count=count) == count and c.field_hashes(3, first=first, count=count) == count
        assert c.line_hashes(first, count) == count

        # distinct_lines is line_hashes over the file, then releases the hashes; it holds numbers only when asked to
        c.hold_line_ranges()
        assert c.distinct_lines(0) == len(e["first_occurrences"])
        assert c.take_line_ranges_is_refused()
        assert c.take_line_hashes(4)[0] == INVALID_ARGUMENT and c.take_distinct_lines(4)[0] == INVALID_ARGUMENT
        assert c.line_hashes_device() is None
        assert c.distinct_lines(1, seed=1) == len(e["first_occurrences"])
        assert c.take_line_hashes(4)[0] == INVALID_ARGUMENT
        wanted = (OK, e["first_occurrences"])
        assert c.take_distinct_lines(len(wanted[1])) == wanted and c.take_distinct_lines(len(wanted[1])) == wanted
        assert c.take_distinct_lines(3) == (OK, wanted[1][:3])
        # ... and it leaves the field families alone
        assert c.take_field_spans(count) == (OK, window_spans) and c.take_field_hashes(count) == (OK, window_keys)
        # the distinct numbers go with the next line_hashes
        assert c.line_hashes(first, count) == count
        assert c.take_distinct_lines(3)[0] == INVALID_ARGUMENT
        assert c.take_line_hashes(count) == (OK, e["hashes"][0][first:first + count])

        # field_groups is field_hashes over the range, then releases the field hashes and holds the groups
        c.hold_line_ranges()
        before = c.launches()
        assert c.field_groups(3) == (len(lines), missing)
        assert c.launches() - before >= 2
        assert c.take_line_ranges_is_refused()
        assert c.take_field_hashes(4)[0] == INVALID_ARGUMENT
        wanted = (OK, [lines, counts, [spans[k][0] for k in lines], [spans[k][1] for k in lines]])
        assert c.take_field_groups(len(lines)) == wanted and c.take_field_groups(len(lines)) == wanted
        assert c.take_field_groups(2) == (OK, [column[:2] for column in wanted[1]])
        # ... and leaves hashes and field spans alone
        assert c.take_line_hashes(count) == (OK, e["hashes"][0][first:first + count])
        assert c.take_field_spans(count) == (OK, window_spans)
        # field_spans and line_hashes leave the groups; field_hashes and field_groups release them
        assert c.field_spans(3, first=first, count=count) == count and c.line_hashes(first, count) == count
        assert c.take_field_groups(len(lines)) == wanted
        assert c.field_hashes(3, first=first, count=count) == count
        assert c.take_field_groups(2)[0] == INVALID_ARGUMENT
        assert c.take_field_hashes(count) == (OK, window_keys)
        window = R.groups_of(e["values"][(3, TAB)], first, count)
        assert c.field_groups(3, first=first, count=count) == (len(window[0]), window[2])
        assert c.take_field_hashes(4)[0] == INVALID_ARGUMENT
        assert c.take_field_groups(len(window[0]))[1][:2] == [window[0], window[1]]
        assert f.tell() == 0


def test_empty_ranges_and_the_device_pointer(native, corpus, monkeypatch):
    e, path = corpus
    monkeypatch.delenv("MI355X_BZ2_READER_CONTEXTS", raising=False)
    monkeypatch.delenv("MI355X_BZ2_INPUT_BUDGET", raising=False)
    n = len(e["lines"])
    first, count = window_on_a_seam(e)
    untouched = [UNTOUCHED] * 3
    with native.open(path, parallelization=PARALLELIZATION) as f:
        c = Calls(native, f)
        # a range that selects no line holds an empty result: the take succeeds with 0 values
        for empty in ((n + 5, 3), (7, 0), (n, ALL)):
            assert c.line_hashes(first, count) == count and c.line_hashes(*empty) == 0
            assert c.take_line_hashes(0) == (OK, []) and c.take_line_hashes(3) == (OK, untouched)
            assert c.field_spans(3, first=first, count=count) == count and c.field_spans(3, TAB, *empty) == 0
            assert c.take_field_spans(0)[0] == OK and c.take_field_spans(3) == (OK, list(zip(untouched, untouched)))
            assert c.field_hashes(3, first=first, count=count) == count and c.field_hashes(3, TAB, 0, *empty) == 0
            assert c.take_field_hashes(0) == (OK, []) and c.take_field_hashes(3) == (OK, untouched)
            assert c.field_groups(3, TAB, 0, *empty) == (0, 0)
            assert c.take_field_groups(0)[0] == OK and c.take_field_hashes(0)[0] == INVALID_ARGUMENT
        # line_hashes_device: the held hashes, for keep_on_device with at least one line
        assert c.line_hashes(n + 5, 3, keep=1) == 0 and c.line_hashes_device() is None
        assert c.line_hashes(keep=0) == n and c.line_hashes_device() is None
        assert c.line_hashes(keep=1) == n and c.line_hashes_device() is not None
        assert c.take_line_hashes(n) == (OK, e["hashes"][0])
        assert c.line_hashes(first, count, seed=1, keep=1) == count and c.line_hashes_device() is not None
        assert c.take_line_hashes(count) == (OK, e["hashes"][1][first:first + count])
        assert c.distinct_lines(0) == len(e["first_occurrences"]) and c.line_hashes_device() is None
        assert f.tell() == 0
