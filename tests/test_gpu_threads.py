"""Callers on several threads inside the C ABI at once: ctypes releases the GIL, so two Python threads that each hold a
reader, a Decoder or nothing but the module functions of buffers.py are in the library together.  What they share there
is listed in DESIGN.md, "Callers on several threads": the walk chain of the device with its mutex, its ring of events and
`liveContexts` -- which every batch reads for its lane layout and its crowd mode --, the once-per-device block of
mi355x_bz2_create, HIP's per-thread current device, the null stream of bz2_distinct.hip, and the kept context and the two
locks of buffers.py.

Every thread uses a reader or Decoder of its own (the contract: one thread at a time per object); every value is compared
with the models (readershapes.expected, columnshapes.expected), with the raw bytes, or with one serial run of the same
calls.  The environment is fixed on the main thread before the workers start and not touched while they run: the library
reads it per batch.  threadrun.py is the harness; test_threadrun.py shows on the CPU that a wrong answer on one thread
fails these tests by thread and operation.

The times in the docstrings are those the tests print on an MI355X; with THREADS_TEST_SERIAL=1 in the environment
a test runs its threads' lists once more on the main thread, one after the other, and prints that time too."""
import bz2
import ctypes
import json
import os
import random
import subprocess
import sys
import threading
import time

import pytest

import threadrun as T
from test_gpu_column_shapes import world as columns_world            # noqa: F401 (fixtures, under names of their own here)
from test_gpu_lanes import records, workload                         # noqa: F401
from test_gpu_reader_shapes import range_of
from test_gpu_reader_shapes import world as reader_world             # noqa: F401

pytestmark = pytest.mark.gpu

DEADLINE = 120                                       # seconds: a guard against a hang, never a performance assertion
HANDOFF = 60                                         # ... and for one wait of a scripted hand-off
SERIAL = os.environ.get("THREADS_TEST_SERIAL") == "1"     # (a switch of these tests, none of the library's)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worlds(reader_world, columns_world):             # noqa: F811
    """{"reader": {variant: e}, "columns": {variant: e}}: computed once, on the main thread, before any worker starts."""
    return {"reader": {v: T.extend_reader_world(reader_world[v]) for v in ("tail", "closed")},
            "columns": {v: T.extend_columns_world(columns_world[v]) for v in ("tail", "closed")}}


def fix_environment(monkeypatch, forced=None):
    if forced is None:
        monkeypatch.delenv("MI355X_BZ2_READER_CONTEXTS", raising=False)
    else:
        monkeypatch.setenv("MI355X_BZ2_READER_CONTEXTS", str(forced))
    monkeypatch.delenv("MI355X_BZ2_INPUT_BUDGET", raising=False)


def serial_seconds(lists):
    """The lists once more, one after the other on this thread -> seconds (only with THREADS_TEST_SERIAL=1)."""
    began = time.monotonic()
    for operations in lists:
        T.run_operations(T.Progress(), operations)
    return time.monotonic() - began


def wait(event):
    assert event.wait(HANDOFF), "the hand-off never came"


# ------------------------------------------------------------------------------------------------ readers side by side

ROWS = [(1, (64, 0)), (None, (3, 64, 0, 5)), (None, (3, 64, 0, 5, 64, 3, 0, 1))]


@pytest.mark.parametrize("forced,parallelizations", ROWS, ids=lambda v: "contexts%s" % v if not isinstance(v, tuple) else "%dthreads" % len(v))
def test_readers_side_by_side(native, worlds, monkeypatch, forced, parallelizations):
    """K threads, each with a reader of its own that the main thread opened, call and compare: every family once (the
    group-bys and the distinct lines sort on the null stream all threads share), 16 seeded operations from the call-order
    lists of the two shape tests, and the whole file by read() -- 25 operations, 9 for the thread at parallelization 1.

      2 threads, one context each: each batch runs on its share of the lanes while the other's walks enter the same chain
      4 threads, about ten contexts: crowd mode, launch caps 3, 64, 512 and 5
      8 threads: the crowd, and eight threads' null-stream sorts interleaved

    On an MI355X, in two runs: 2 threads 0.51 - 0.74 s with an overlap share of 0.68, 4 threads 1.23 - 2.34 s (0.92 - 0.93),
    8 threads 3.70 - 5.07 s (0.97), the thread at parallelization 1 being the last to finish.  The same lists once more on
    one thread, the readers' indexes then built and their input resident: 0.24, 1.49 - 2.62 and 4.31 - 5.12 s."""
    fix_environment(monkeypatch, forced)
    readers, lists, report = [], [], None
    try:
        for index, parallelization in enumerate(parallelizations):
            f, operations = T.thread_operations(native.open, worlds, index, parallelization, 0 if parallelization == 1 else 16, native)
            readers.append(f)
            lists.append(operations)
        report = T.run_threads([lambda progress, operations=operations: T.run_operations(progress, operations) for operations in lists], DEADLINE)
        share = T.overlap_share(report)
        print("side by side, %d threads: %.2f s, overlap share %.2f, per thread %s" % (
            len(lists), T.wall_time(report), share, ["%.2f" % sum(t1 - t0 for _, t0, t1 in r.operations) for r in report]))
        T.assert_clean(report)
        assert [r.result for r in report] == [len(operations) for operations in lists]
        assert share >= 0.5, "the run was serial: it shows nothing about threads"
        for f in readers:
            assert f.tell() == 0                     # (the last operation leaves it there)
        if SERIAL:
            print("  the same on one thread: %.2f s" % serial_seconds(lists))
    finally:
        T.close_unless_stuck(report, readers)        # (a stuck thread is still inside its reader: then none is closed)


CHURN_PARALLELIZATIONS = (3, 64, 0, 5)


def test_open_query_close_churn(native, worlds, monkeypatch):
    """4 threads, 6 rounds each of: open a reader (parallelization 3, 64, 0, 5 in turn, each thread starting elsewhere),
    three seeded operations, close -- one barrier at the start and none after it, so contexts are created and destroyed
    while other threads' batches are in flight, and `liveContexts` moves under them.

    On an MI355X, in two runs: 2.64 - 3.67 s, overlap share 0.99 - 1.00; the same 24 rounds on one thread 4.51 - 4.75 s."""
    fix_environment(monkeypatch)

    def churn(index):
        def work(progress):
            rng = random.Random(T.THREADS_SEED * 1_000 + 100 + index)
            done = 0
            for round_ in range(6):
                parallelization = CHURN_PARALLELIZATIONS[(index + round_) % 4]
                with progress.operation("round %d: open(parallelization=%d)" % (round_, parallelization)):
                    f, operations = T.churn_operations(native.open, worlds, index + round_, parallelization, rng, native)
                try:
                    done += T.run_operations(progress, [("round %d: %s" % (round_, label), call, want) for label, call, want in operations])
                finally:
                    with progress.operation("round %d: close" % round_):
                        f.close()
            return done
        return work

    report = T.run_threads([churn(index) for index in range(4)], DEADLINE)
    share = T.overlap_share(report)
    print("churn, 4 threads: %.2f s, overlap share %.2f" % (T.wall_time(report), share))
    T.assert_clean(report)
    assert [r.result for r in report] == [18] * 4
    assert share >= 0.5
    if SERIAL:
        began = time.monotonic()
        for index in range(4):
            churn(index)(T.Progress())
        print("  the same on one thread: %.2f s" % (time.monotonic() - began))


def test_held_results_per_thread(native, worlds, monkeypatch):
    """Result buffers belong to a context: thread A holds line ranges in its reader's contexts (step 1 of read_line_ranges)
    while thread B runs a whole-file grep_regex on its own reader, then takes them; then B holds selected lines (step 1 of
    select_lines) across a whole-file grep_regex of A.  The hand-offs are events: the order is the same in every run.
    (The tensor forms of the two calls: test_tensor_calls_on_threads_in_a_fresh_process.)

    On an MI355X: 0.22 - 0.24 s.  The hand-offs put the steps one after the other, so this is the one-thread time as well,
    and no overlap share is asserted."""
    fix_environment(monkeypatch)
    ea, eb = worlds["reader"]["tail"], worlds["columns"]["closed"]
    ranges = [(5, 3), (ea["n"] - 2, 10), (1_000, 40)]
    want_ranges = b"".join(range_of(ea, first, count) for first, count in ranges)
    selected = [k for k, flag in enumerate(eb["flags"]["get"]) if flag]
    want_selected = b"".join(eb["whole_lines"][k] for k in selected)
    want_regex_a, want_regex_b = ea["regex"][(T.READER_REGEX, False)], eb["regex_lines"]
    a_holds, b_searched, b_holds, a_searched = (threading.Event() for _ in range(4))

    def regex(f, pattern):
        numbers, lines = f.grep_regex(pattern)
        return numbers.tolist(), lines

    def take(f, total):
        destination = ctypes.create_string_buffer(max(total, 1))
        assert native.lib().mi355x_bz2_reader_take_line_ranges(f._open_reader()._h, destination, 0) == 0
        return destination.raw[:total]

    fa, fb, report = native.open(ea["path"], parallelization=64), native.open(eb["path"], parallelization=5), None
    try:
        def thread_a(progress):
            try:
                with progress.operation("A: hold line ranges"):
                    sizes, total = fa._open_reader()._read_line_ranges(ranges, b"\n", False)
                a_holds.set()
                with progress.operation("A: wait for B's grep_regex"):
                    wait(b_searched)
                with progress.operation("A: take line ranges"):
                    assert sum(sizes) == total == len(want_ranges) and take(fa, total) == want_ranges
                with progress.operation("A: wait for B's hold"):
                    wait(b_holds)
                with progress.operation("A: grep_regex under B's hold"):
                    assert regex(fa, T.READER_REGEX) == want_regex_a
            finally:
                a_holds.set()                        # (a failure above must not leave B waiting for its hand-off)
                a_searched.set()
            return "a"

        def thread_b(progress):
            try:
                with progress.operation("B: wait for A's hold"):
                    wait(a_holds)
                with progress.operation("B: grep_regex under A's hold"):
                    assert regex(fb, T.COLUMNS_REGEX) == want_regex_b
                b_searched.set()
                with progress.operation("B: hold selected lines"):
                    reader = fb._open_reader()
                    held, _, total = reader._select_lines(reader._where_arguments(1, [b"GET"], None, False, 0, None, None, b"\t", b"\n", 0), False)
                b_holds.set()
                with progress.operation("B: wait for A's grep_regex"):
                    wait(a_searched)
                with progress.operation("B: take selected lines"):
                    assert held.tolist() == selected and total == len(want_selected) and take(fb, total) == want_selected
            finally:
                b_searched.set()
                b_holds.set()
            return "b"

        report = T.run_threads([thread_a, thread_b], DEADLINE)
        print("held results: %.2f s" % T.wall_time(report))
        T.assert_clean(report)
        assert [r.result for r in report] == ["a", "b"]
    finally:
        T.close_unless_stuck(report, [fa, fb])


# ------------------------------------------------------------------------------------------------ decoders side by side

def serial_run(native, workload):                                      # noqa: F811
    """One Decoder, one batch, on this thread -> the records every other run must equal."""
    enc, raw, offsets = workload
    n = len(offsets)
    with_pinned = (ctypes.c_ubyte * len(enc)).from_buffer_copy(enc)
    decoder = native.Decoder(max_batch_blocks=n)
    try:
        offs, res = decoder.make_arrays(offsets)
        decoder.set_input_host_async(ctypes.addressof(with_pinned), len(enc), keepalive=with_pinned)
        decoder.begin_batch(offs, n)
        total = decoder.end_batch(res)
        want = records(res, n)
        assert total == len(raw) and decoder.copy_output(0, total) == raw
        assert all(r["status"] == 0 and r["computed_crc"] == r["header_crc"] for r in want)
    finally:
        decoder.close()
    return with_pinned, want


def kept_context_alive(native):
    """The kept context of buffers.py counts among the contexts alive on the device from the first call of a module
    function on, for the rest of the process.  With it created here the decoder tests below start from one and the same
    count whatever ran before them: it, and the Decoders they create themselves (every reader and Decoder of the tests
    in front of them is closed)."""
    assert native.decompress(bz2.compress(b"kept")) == b"kept"


def slowest(report):
    """{label: the longest time any thread spent in it}, for the lines the tests print."""
    longest = {}
    for r in report:
        for label, t0, t1 in r.operations:
            longest[label] = max(longest.get(label, 0.0), t1 - t0)
    return ", ".join("%s %.3f" % item for item in longest.items())


class Batches:
    """A Decoder of the calling thread over the shared pinned input: begin, and end with the comparison."""

    def __init__(self, native, workload, pinned, want):                 # noqa: F811
        self.enc, self.raw, self.offsets = workload
        self.pinned, self.want, self.n = pinned, want, len(self.offsets)
        self.decoder = native.Decoder(max_batch_blocks=self.n)
        self.offs, self.res = self.decoder.make_arrays(self.offsets)
        self.queue_input()

    def queue_input(self):
        self.decoder.set_input_host_async(ctypes.addressof(self.pinned), len(self.enc), keepalive=self.pinned)

    def begin(self):
        self.decoder.begin_batch(self.offs, self.n)

    def end(self, where):
        total = self.decoder.end_batch(self.res)
        got = records(self.res, self.n)
        assert total == len(self.raw), where
        assert all(r["status"] == 0 and r["computed_crc"] == r["header_crc"] for r in got), where
        assert got == self.want, where
        assert self.decoder.copy_output(0, total) == self.raw, where

    def close(self):
        self.decoder.close()


@pytest.mark.parametrize("threads", (1, 2, 3, 5))
def test_decoders_on_threads(native, workload, threads):                # noqa: F811
    """The batch of test_gpu_lanes.py (324 level-1 blocks), two rounds on every thread's own Decoder, created on that
    thread; the first round queues the context's next input while its batch runs.  Records, CRCs and the bytes of
    copy_output equal one serial run, for every thread and round.  The kept context of buffers.py is alive as well
    (kept_context_alive), so with 1, 2, 3 and 5 threads up to 2, 3, 4 and 6 contexts are alive: a batch runs on 2, 1, 1 and
    1 lanes, from 2 threads on in crowd mode -- and the contexts appear while other threads' batches are in flight.

    On an MI355X: 0.06, 0.08, 0.12 and 0.20 s for 1, 2, 3 and 5 threads (one thread: 0.06 s per decoder), overlap share
    0.97 - 1.00 from 2 threads on; the longest create 0.008, 0.013, 0.025 and 0.043 s, the longest end_batch with its
    comparison 0.023, 0.029, 0.035 and 0.071 s.  Now and then the whole is far longer -- 0.82 s with 3 threads in one
    run, 1.35 s with 5 in another -- and then it is the create: 1.17 s of those 1.35 s, five contexts allocating their
    3.3 GB of scratch side by side, against 0.1 s for each batch."""
    kept_context_alive(native)
    pinned, want = serial_run(native, workload)

    def worker(index):
        def work(progress):
            with progress.operation("create"):
                batches = Batches(native, workload, pinned, want)
            try:
                for round_ in range(2):
                    with progress.operation("round %d: begin_batch" % round_):
                        batches.begin()
                        if round_ == 0:
                            batches.queue_input()
                    with progress.operation("round %d: end_batch and compare" % round_):
                        batches.end((threads, index, round_))
            finally:
                with progress.operation("close"):
                    batches.close()
            return index
        return work

    report = T.run_threads([worker(index) for index in range(threads)], DEADLINE)
    print("decoders on %d threads: %.2f s, overlap share %.2f; the longest of each step: %s" % (
        threads, T.wall_time(report), T.overlap_share(report), slowest(report)))
    T.assert_clean(report)
    assert [r.result for r in report] == list(range(threads))
    assert threads == 1 or T.overlap_share(report) >= 0.5


@pytest.mark.parametrize("case", ("created", "destroyed", "destroyed-in-crowd"))
def test_context_created_and_destroyed_under_a_batch_in_flight(native, workload, case):     # noqa: F811
    """`liveContexts`, the lane budget and the walk chain move between one thread's begin_batch and its end_batch, in a
    fixed order (hand-offs through events).  The kept context of buffers.py is alive throughout (kept_context_alive), so
    the counts are the same in every session:

      created             two alive (the kept one and A's): A begins, without the crowd; B creates a decoder -- the third,
                          the crowd threshold is crossed upwards -- and begins and ends a batch of its own; A ends
      destroyed           three alive (the kept one, A's, B's): A begins in crowd mode; B closes its decoder, two are left
                          and the threshold is crossed downwards; A ends
      destroyed-in-crowd  four alive (B has two): A begins; B closes one, three are left, still a crowd; A ends

    In the last two A then runs a second batch, planned for the count that is left, beside one of B's where B has a
    decoder left.  Every result equals the serial run's records and bytes.

    On an MI355X: 0.06, 0.10 and 0.09 s; the hand-offs put the steps one after the other but for the second batches, so
    these are one-thread times as well.  A batch that ends after the other thread's create or close: 0.010 - 0.020 s."""
    kept_context_alive(native)
    pinned, want = serial_run(native, workload)
    a_ready, b_ready, a_began, b_done = (threading.Event() for _ in range(4))

    def thread_a(progress):
        with progress.operation("A: create"):
            batches = Batches(native, workload, pinned, want)
        try:
            a_ready.set()
            with progress.operation("A: wait for B to be ready"):
                wait(b_ready)
            with progress.operation("A: begin_batch"):
                batches.begin()
                batches.queue_input()
            a_began.set()
            with progress.operation("A: wait for B"):
                wait(b_done)
            with progress.operation("A: end_batch and compare"):
                batches.end((case, "A"))
            if case != "created":
                with progress.operation("A: second batch, after B's close"):
                    batches.begin()
                    batches.end((case, "A, second batch"))
        finally:
            a_ready.set()                            # (a failure above must not leave B waiting for its hand-off)
            a_began.set()
            with progress.operation("A: close"):
                batches.close()
        return "a"

    def thread_b(progress):
        mine = []
        try:
            with progress.operation("B: wait for A's decoder"):
                wait(a_ready)
            if case != "created":
                with progress.operation("B: create"):
                    mine = [Batches(native, workload, pinned, want) for _ in range(2 if case == "destroyed-in-crowd" else 1)]
            b_ready.set()
            with progress.operation("B: wait for A's begin_batch"):
                wait(a_began)
            if case == "created":
                with progress.operation("B: create under A's batch"):
                    mine = [Batches(native, workload, pinned, want)]
                with progress.operation("B: a batch of its own under A's"):
                    mine[0].begin()
                    mine[0].end((case, "B"))
            else:
                with progress.operation("B: close under A's batch"):
                    mine.pop().close()
            b_done.set()
            if mine and case != "created":
                with progress.operation("B: a batch beside A's second"):
                    mine[0].begin()
                    mine[0].end((case, "B"))
        finally:
            b_ready.set()
            b_done.set()
            with progress.operation("B: close"):
                for batches in mine:
                    batches.close()
        return "b"

    report = T.run_threads([thread_a, thread_b], DEADLINE)
    print("context %s under a batch: %.2f s; %s" % (case, T.wall_time(report), slowest(report)))
    T.assert_clean(report)
    assert [r.result for r in report] == ["a", "b"]


# ------------------------------------------------------------------------------------------------ the module functions

def thread_buffers(index):
    """Six raw buffers of thread `index`, 0 to 300 000 bytes, the empty one and a single byte among them; their .bz2 forms,
    one of them damaged in the middle of its block."""
    rng = random.Random(T.THREADS_SEED * 1_000 + 200 + index)
    words = [bytes(rng.choices(b"abcdefghij \n", k=rng.randrange(2, 9))) for _ in range(200)]

    def text(size):
        return b" ".join(rng.choices(words, k=size // 4 + 1))[:size]

    raws = [b"", bytes([rng.randrange(256)]), text(300_000), text(rng.randrange(2, 5_000)), rng.randbytes(rng.randrange(1_000, 120_000)),
            text(rng.randrange(100_000, 250_000))]
    rng.shuffle(raws)
    encoded = [bz2.compress(raw, rng.choice([1, 9])) for raw in raws]
    damaged = max(range(6), key=lambda k: (len(raws[k]) < 200_000, len(raws[k])))          # the largest below 200 000 bytes
    broken = bytearray(encoded[damaged])
    broken[len(broken) // 2] ^= 0xFF
    encoded[damaged] = bytes(broken)
    return raws, encoded, damaged


def compress_input(raws, damaged):
    """The buffer that `compress` gets: the last one whose .bz2 form is undamaged."""
    return raws[[k for k in range(6) if k != damaged][-1]]


def buffer_calls(native, raws, encoded, damaged):
    """{name: call} of the module functions over one thread's buffers, each returning plain values."""
    good = [k for k in range(6) if k != damaged]

    def many():
        out, statuses = native.decompress_many(encoded, return_status=True)
        return out, statuses.tolist()

    def compress_many(level):
        return lambda: native.compress_many(raws, level, return_index=True)

    return {"decompress_many": many, "decompress": lambda: [native.decompress(encoded[k]) for k in good[:2]],
            "compress_many(1)": compress_many(1), "compress_many(9)": compress_many(9),
            "compress": lambda: native.compress(compress_input(raws, damaged), 5)}


def test_buffers_functions_from_four_threads(native, worlds, monkeypatch):
    """decompress_many, decompress, compress_many with the index at levels 1 and 9 and compress (decompress_many_to_tensor:
    test_tensor_calls_on_threads_in_a_fresh_process), in a seeded order on each of four threads, each over six buffers of
    its own (one damaged: statuses, not an exception), while a fifth thread runs reader queries: the kept context of
    buffers.py behind its lock.  Wanted are the raw buffers, and what one serial call of each returned before the threads
    started -- for compression byte for byte, index included, and bz2.decompress gives the input back.

    On an MI355X: 0.70 s for the five threads, overlap share 1.00; the serial calls in front of them 0.84 s, the
    generation of the buffers included."""
    fix_environment(monkeypatch)
    began = time.monotonic()
    sets, wanted = [], []
    for index in range(4):
        raws, encoded, damaged = thread_buffers(index)
        calls = buffer_calls(native, raws, encoded, damaged)
        want = {name: call() for name, call in calls.items()}
        clean = [b"" if k == damaged else raw for k, raw in enumerate(raws)]
        out, statuses = want["decompress_many"]
        assert out == clean and [s != 0 for s in statuses] == [k == damaged for k in range(6)], (index, statuses)
        assert want["decompress"] == [raws[k] for k in range(6) if k != damaged][:2]
        for level in (1, 9):
            assert [bz2.decompress(blob) for blob, _ in want["compress_many(%d)" % level]] == raws
        assert bz2.decompress(want["compress"]) == compress_input(raws, damaged)
        sets.append((raws, calls, damaged))
        wanted.append(want)
    serial = time.monotonic() - began

    def worker(index):
        def work(progress):
            raws, calls, damaged = sets[index]
            order = sorted(calls)
            random.Random(T.THREADS_SEED * 1_000 + 300 + index).shuffle(order)
            for name in order:
                with progress.operation(name):
                    got = calls[name]()
                    assert got == wanted[index][name], name
                    if name.startswith("compress_many"):
                        assert [bz2.decompress(blob) for blob, _ in got] == raws, name
                    if name == "compress":
                        assert bz2.decompress(got) == compress_input(raws, damaged), name
            return order
        return work

    f, operations = T.thread_operations(native.open, worlds, 0, 64, 8, native)
    report = None
    try:
        report = T.run_threads([worker(index) for index in range(4)] + [lambda progress: T.run_operations(progress, operations)], DEADLINE)
    finally:
        T.close_unless_stuck(report, [f])
    share = T.overlap_share(report)
    print("module functions, 4 threads and a reader: %.2f s, overlap share %.2f; the serial calls (generation included) %.2f s" % (
        T.wall_time(report), share, serial))
    T.assert_clean(report)
    assert all(sorted(r.result) == sorted(sets[0][1]) for r in report[:4]) and len({tuple(r.result) for r in report[:4]}) > 1
    assert share >= 0.5


CHILD = r"""
import hashlib, json, os, sys, threading, time
sys.path.insert(0, sys.argv[1])
import indexed_bzip2_amd as m
buffers = json.load(open(sys.argv[2]))
warm = m.warmup()                                      # its daemon thread initialises the runtime while the others start
results, failures = {}, {}
serial = sys.argv[4:] == ["serial"]                     # the same calls one after the other, for the one-thread time
barrier = threading.Barrier(1 if serial else 5)

def guarded(name, call):
    def body():
        try:
            barrier.wait(60)
            results[name] = hashlib.sha256(call()).hexdigest()
        except BaseException as failure:
            failures[name] = repr(failure)
    return threading.Thread(target=body, daemon=True, name=name)

def read_all():
    with m.open(sys.argv[3], 4) as f:
        return f.read()

threads = [guarded("decompress %d" % k, lambda k=k: m.decompress(bytes.fromhex(buffers[k]))) for k in range(4)] + [guarded("reader", read_all)]
deadline = time.monotonic() + 90
for thread in threads:
    thread.start()
    if serial:
        thread.join(max(0.0, deadline - time.monotonic()))
for thread in threads + [warm]:
    thread.join(max(0.0, deadline - time.monotonic()))
stuck = [thread.name for thread in threads + [warm] if thread.is_alive()]
print(json.dumps({"results": results, "failures": failures, "stuck": stuck}))
sys.stdout.flush()
os._exit(3 if stuck else 1 if failures else 0)          # (a stuck daemon thread must not keep the interpreter from ending)
"""


def run_child(name, arguments):
    """The child process, waited for with a timeout -> its CompletedProcess.  One that ran into the timeout, ended by a
    signal or reports a stuck thread (status 3) ends the session as a stuck thread of this process does."""
    began = time.monotonic()
    try:
        child = subprocess.run([sys.executable, "-c"] + arguments, timeout=DEADLINE, capture_output=True, text=True)
    except subprocess.TimeoutExpired as expired:
        pytest.exit("the child process of %s ran into its timeout: %s" % (name, expired.stderr), returncode=T.STUCK_RETURNCODE)
    print("%s: the child took %.2f s" % (name, time.monotonic() - began))
    if child.returncode < 0 or child.returncode == T.STUCK_RETURNCODE:
        pytest.exit("the child process of %s ended with status %d: %s\n%s" % (name, child.returncode, child.stdout, child.stderr),
                    returncode=T.STUCK_RETURNCODE)
    assert child.returncode == 0, (child.returncode, child.stdout, child.stderr)
    return json.loads(child.stdout.strip().splitlines()[-1])


def test_first_calls_in_a_fresh_process(native, tmp_path):
    """One child process: warmup() on its daemon thread, four threads whose first act is decompress -- they race the lazy
    creation of the kept context in buffers._decoder and the once-per-device block of mi355x_bz2_create -- and one thread
    that opens a reader and reads.  The child prints the SHA-256 of every result; a child that ends by a signal, runs into
    the timeout or reports a stuck thread ends the session as a stuck thread here does.

    On an MI355X: 0.3 - 0.5 s for the child; 0.6 s for a child that makes the same calls one after the other."""
    import hashlib
    from conftest import FIXTURES
    rng = random.Random(T.THREADS_SEED)
    raws = [bytes(rng.choices(b"abcdefgh \n", k=size)) for size in (1, 40_000, 250_000, 1_200_000)]
    (tmp_path / "buffers.json").write_text(json.dumps([bz2.compress(raw, 9 if k % 2 else 1).hex() for k, raw in enumerate(raws)]))
    path = os.path.join(FIXTURES, "base64-256KiB.bz2")
    with open(os.path.join(FIXTURES, "base64-256KiB"), "rb") as fixture:
        whole = fixture.read()
    want = {"decompress %d" % k: hashlib.sha256(raw).hexdigest() for k, raw in enumerate(raws)}
    want["reader"] = hashlib.sha256(whole).hexdigest()
    for mode in ([], ["serial"]) if SERIAL else ([],):
        answer = run_child("test_first_calls_in_a_fresh_process%s" % mode, [CHILD, ROOT, str(tmp_path / "buffers.json"), path] + mode)
        assert answer["failures"] == {} and answer["stuck"] == []
        assert answer["results"] == want


# ------------------------------------------------------------------------------------------------ the tensor calls

TENSOR_CHILD = r"""
import torch                      # first: one HIP runtime in the process, as bench.py does
torch.zeros(1, device="cuda")
import os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import test_gpu_threads
test_gpu_threads.tensor_threads_main(sys.argv[2], sys.argv[3:] == ["serial"])
"""


def tensor_threads_main(folder, serial=False):
    """The body of the child of test_tensor_calls_on_threads_in_a_fresh_process: prints one JSON line and ends the process
    with status 0, 1 (a thread failed) or 3 (a thread is stuck).  `serial`: the lists once more on the main thread."""
    import numpy as np
    import indexed_bzip2_amd as native
    e = T.plain_reader_world(("tail",))["tail"]
    e["path"] = os.path.join(folder, "tail.bz2")
    with open(e["path"], "wb") as out:
        out.write(e["enc"])
    world = {"reader": {"tail": e, "closed": e}}
    ranges = [(5, 3), (e["n"] - 2, 10), (1_000, 40)]
    want_ranges = [range_of(e, first, count) for first, count in ranges]
    want_selected = b"".join(range_of(e, k, 1) for k in e["selected"])
    want_regex = e["regex"][(T.READER_REGEX, False)]
    # the hand-offs between threads 0 and 1: each keeps a tensor across a whole-file grep_regex of the other
    kept_0, searched_1, kept_1, searched_0 = (threading.Event() for _ in range(4))

    def as_bytes(tensor):
        assert tensor.is_cuda
        return tensor.cpu().numpy().tobytes()

    def tensor_operations(f, index):
        """(read_line_ranges_to_tensor, select_lines_to_tensor, decompress_many_to_tensor, the first one's tensor again, the
        second one's again, a whole-file grep_regex) of thread `index`."""
        raws, encoded, damaged = thread_buffers(10 + index)
        clean = [b"" if k == damaged else raw for k, raw in enumerate(raws)]
        kept = {}

        def line_ranges():
            kept["ranges"], offsets = f.read_line_ranges_to_tensor(ranges)
            return as_bytes(kept["ranges"]), offsets.tolist()

        def selected_lines():
            numbers, kept["selected"], _ = f.select_lines_to_tensor(1, values=list(T.READER_KEYS))
            return numbers.tolist(), as_bytes(kept["selected"])

        def many():
            data, offsets, statuses = native.decompress_many_to_tensor(encoded, return_status=True)
            return as_bytes(data), offsets.tolist(), [status != 0 for status in statuses.tolist()]

        def regex():
            numbers, lines = f.grep_regex(T.READER_REGEX)
            return numbers.tolist(), lines

        return [("read_line_ranges_to_tensor", line_ranges, (b"".join(want_ranges), np.cumsum([0] + [len(r) for r in want_ranges]).tolist())),
                ("select_lines_to_tensor", selected_lines, (e["selected"], want_selected)),
                ("decompress_many_to_tensor", many, (b"".join(clean), np.cumsum([0] + [len(c) for c in clean]).tolist(), [k == damaged for k in range(6)])),
                ("the tensor of read_line_ranges_to_tensor, again", lambda: as_bytes(kept["ranges"]), b"".join(want_ranges)),
                ("the tensor of select_lines_to_tensor, again", lambda: as_bytes(kept["selected"]), want_selected),
                ("grep_regex, whole file", regex, want_regex)]

    def then_set(operation, event):
        label, call, want = operation

        def call_and_set():
            got = call()
            event.set()
            return got
        return label, call_and_set, want

    def behind(event, operation, what):
        label, call, want = operation
        return "%s, behind %s" % (label, what), lambda: (event.wait(20), call()), (True, want)      # (two such waits fit the deadline)

    readers, lists = [], []
    for index, parallelization in enumerate((3, 64, 0, 5)):
        f, operations = T.thread_operations(native.open, world, index, parallelization, 4, native, tensors=True)
        ranges_op, selected_op, many_op, ranges_again, selected_again, regex_op = tensor_operations(f, index)
        readers.append(f)
        if index == 0:
            head = [then_set(ranges_op, kept_0), behind(searched_1, ranges_again, "thread 1's grep_regex"),
                    then_set(behind(kept_1, regex_op, "thread 1's select_lines_to_tensor"), searched_0)]
            tail = [selected_op, many_op, ranges_again]
        elif index == 1:
            head = [then_set(behind(kept_0, regex_op, "thread 0's read_line_ranges_to_tensor"), searched_1), then_set(selected_op, kept_1),
                    behind(searched_0, selected_again, "thread 0's grep_regex"), ranges_op]
            tail = [many_op, ranges_again]
        else:
            head, tail = [ranges_op], [selected_op, many_op, ranges_again]        # the kept tensor spans the thread's other calls
        lists.append(head + operations[:-1] + tail + operations[-1:])
    report = T.run_threads([lambda progress, operations=operations: T.run_operations(progress, operations) for operations in lists], 90)
    answer = {"failed": ["thread %d failed in %s: %s" % (r.index, r.label, r.trace) for r in report if r.exception is not None],
              "stuck": ["thread %d is stuck in %s" % (r.index, r.stuck) for r in report if r.stuck is not None],
              "results": [r.result for r in report], "wanted": [len(operations) for operations in lists],
              "share": T.overlap_share(report), "seconds": T.wall_time(report)}
    if serial and not answer["stuck"] and not answer["failed"]:
        answer["seconds_serial"] = serial_seconds(lists)
    print(json.dumps(answer))
    sys.stdout.flush()
    os._exit(3 if answer["stuck"] else 1 if answer["failed"] else 0)


def test_tensor_calls_on_threads_in_a_fresh_process(native, tmp_path):
    """The *_to_tensor calls from four threads.  They need torch's HIP runtime, which must be the process's first, so
    they run in one child process that imports torch first (as the tensor tests of the other files do): each thread has
    a reader of its own on the corpus of readershapes.py and runs every family with line_hashes_to_tensor, four seeded
    operations, read_line_ranges_to_tensor -- whose tensor is compared again after the thread's other calls --,
    select_lines_to_tensor, and decompress_many_to_tensor over six buffers of its own with one damaged.  Threads 0 and 1
    hand off through events: thread 0 keeps the tensor of read_line_ranges_to_tensor across a whole-file grep_regex of
    thread 1 on its own reader and compares it then, and thread 1 that of select_lines_to_tensor across one of thread 0.

    On an MI355X: 1.76 s for the four threads, overlap share 0.94, and 1.73 s for the same lists on one thread; 6.6 s for
    the child, torch's start and the models of the corpus included."""
    answer = run_child("test_tensor_calls_on_threads_in_a_fresh_process", [TENSOR_CHILD, ROOT, str(tmp_path)] + (["serial"] if SERIAL else []))
    print("tensor calls, 4 threads: %.2f s, overlap share %.2f; on one thread: %s s" % (answer["seconds"], answer["share"], answer.get("seconds_serial")))
    assert answer["failed"] == [] and answer["stuck"] == []
    assert answer["results"] == answer["wanted"] == [8 + 4 + 1 + 6, 8 + 4 + 1 + 6, 8 + 4 + 1 + 4, 8 + 4 + 1 + 4]
    assert answer["share"] >= 0.5
