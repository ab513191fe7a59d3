"""threadrun.py on the CPU: the harness with pure Python stand-ins (time.sleep releases the GIL as a ctypes call does), and
the reader worker loop of test_gpu_threads.py driven with a model reader that answers from readershapes.expected -- with a
correct model the loop passes, with one wrong value in one operation on one thread it fails and names both.  That is the
evidence that the GPU tests fail when an answer is wrong; nothing in the product is broken to show it."""
import threading
import time

import numpy as np
import pytest

import grepgen
import readershapes as R
import threadrun as T
from test_gpu_reader_shapes import groups_of, range_of                    # (pure Python helpers of that file)


# ------------------------------------------------------------------------------------------------ the harness

def sleeper(index, operations=3, seconds=0.02):
    def work(progress):
        for k in range(operations):
            with progress.operation("sleep %d" % k):
                time.sleep(seconds)
        return index * 10
    return work


def test_results_per_thread_and_in_order():
    report = T.run_threads([sleeper(index) for index in range(8)], 10)
    assert [r.index for r in report] == list(range(8))
    assert [r.result for r in report] == [index * 10 for index in range(8)]
    assert all(r.exception is None and r.stuck is None for r in report)
    assert all([label for label, _, _ in r.operations] == ["sleep 0", "sleep 1", "sleep 2"] for r in report)
    assert all(t0 <= t1 for r in report for _, t0, t1 in r.operations)
    assert all(a[2] <= b[1] for r in report for a, b in zip(r.operations, r.operations[1:]))      # one thread's are sequential
    T.assert_clean(report)


def test_exception_in_one_thread_is_reported_with_its_label():
    def failing(progress):
        with progress.operation("fine"):
            time.sleep(0.01)
        with progress.operation("divide"):
            return 1 // 0

    workers = [sleeper(index) for index in range(8)]
    workers[3] = failing
    report = T.run_threads(workers, 10)
    assert isinstance(report[3].exception, ZeroDivisionError) and report[3].label == "divide" and report[3].stuck is None
    assert "ZeroDivisionError" in report[3].trace and "1 // 0" in report[3].trace
    assert [label for label, _, _ in report[3].operations] == ["fine"]
    assert all(r.result == r.index * 10 and r.exception is None and len(r.operations) == 3 for r in report if r.index != 3)
    with pytest.raises(pytest.fail.Exception) as failure:
        T.assert_clean(report)
    assert "thread 3 failed in divide" in str(failure.value) and "thread 2" not in str(failure.value)


def test_the_failing_operation_is_named_whatever_a_finally_clause_runs_after_it():
    def failing(progress):
        try:
            with progress.operation("query"):
                raise ValueError("wrong")
        finally:
            with progress.operation("close"):
                time.sleep(0.01)

    report = T.run_threads([failing], 10)
    assert report[0].label == "query" and isinstance(report[0].exception, ValueError)
    assert [label for label, _, _ in report[0].operations] == ["close"]


def test_exception_between_operations():
    def failing(progress):
        raise KeyError("nothing begun")

    report = T.run_threads([failing, sleeper(1)], 10)
    assert report[0].label is None and isinstance(report[0].exception, KeyError)
    with pytest.raises(pytest.fail.Exception, match="thread 0 failed in " + T.BETWEEN.replace("(", r"\(").replace(")", r"\)")):
        T.assert_clean(report)


def test_stuck_worker_is_reported_and_ends_the_session():
    release = threading.Event()

    def blocked(progress):
        with progress.operation("fine"):
            pass
        with progress.operation("wait for the event"):
            release.wait()
        return "released"

    began = time.monotonic()
    report = T.run_threads([sleeper(0), blocked, sleeper(2)], 0.3)
    took = time.monotonic() - began
    try:
        assert 0.3 <= took < 2.0, took
        assert report[1].stuck == "wait for the event" and report[1].result is None
        assert [label for label, _, _ in report[1].operations] == ["fine"]
        assert report[0].stuck is None and report[2].stuck is None and report[0].result == 0 and report[2].result == 20
        with pytest.raises(pytest.exit.Exception) as ended:
            T.assert_clean(report)
        assert "thread 1 is stuck in wait for the event" in str(ended.value)
        assert ended.value.returncode == T.STUCK_RETURNCODE == 3
    finally:
        release.set()


class Closable:
    """A reader as far as close_unless_stuck goes: close() and the finaliser record that they ran."""

    def __init__(self, log):
        self.log = log

    def close(self):
        self.log.append("close")

    def __del__(self):
        self.log.append("finalised")


def test_no_reader_is_closed_while_a_thread_is_stuck():
    """A stuck worker is still inside its reader: neither that reader nor any other is closed or collected, although
    assert_clean ends the session from inside the try block; with every worker back, all are closed."""
    release = threading.Event()
    log = []

    def blocked(progress):
        with progress.operation("inside the reader"):
            release.wait()

    readers, report = [Closable(log), Closable(log)], None
    try:
        with pytest.raises(pytest.exit.Exception):
            try:
                report = T.run_threads([sleeper(0), blocked], 0.3)
                T.assert_clean(report)
            finally:
                assert T.close_unless_stuck(report, readers) is False
        del readers[:]                                # the last references of this test: the readers must outlive them
        assert log == []
    finally:
        release.set()
    readers, report = [Closable(log), Closable(log)], None
    try:
        report = T.run_threads([sleeper(0), sleeper(1)], 10)
        T.assert_clean(report)
    finally:
        assert T.close_unless_stuck(report, readers) is True
    assert log == ["close", "close"]
    # no threads ran (a failure while the lists were built): closed as well
    assert T.close_unless_stuck(None, [Closable(log)]) is True and log[:3] == ["close"] * 3


def test_the_model_reader_is_left_open_under_a_stuck_worker(model_world):
    """The worker loop with a model reader whose read() never returns: its close() is not called."""
    release = threading.Event()
    closed = []

    class Hanging(ModelReader):
        def read(self, n=None):
            release.wait()
            return ModelReader.read(self, n)

        def close(self):
            closed.append(self.e["path"])

    readers, lists, report = [], [], None
    try:
        for index in range(2):
            kind = Hanging if index == 1 else ModelReader
            f, operations = T.thread_operations(lambda path, _: kind(model_world["reader"][path]), model_world, index, 1, 0, tensors=True)
            readers.append(f)
            lists.append(operations)
        with pytest.raises(pytest.exit.Exception) as ended:
            try:
                report = T.run_threads([lambda progress, operations=operations: T.run_operations(progress, operations) for operations in lists], 1.0)
                T.assert_clean(report)
            finally:
                T.close_unless_stuck(report, readers)
        assert "thread 1 is stuck in " in str(ended.value) and report[0].stuck is None and report[0].result == 9
        assert closed == []
    finally:
        release.set()


def test_one_deadline_for_all_threads():
    """Three blocked workers cost one deadline, not three."""
    release = threading.Event()

    def blocked(progress):
        with progress.operation("wait"):
            release.wait()

    began = time.monotonic()
    report = T.run_threads([blocked] * 3, 0.3)
    took = time.monotonic() - began
    release.set()
    assert [r.stuck for r in report] == ["wait"] * 3 and took < 0.8, took


def span_report(spans_by_thread):
    report = [T.ThreadReport(index) for index in range(len(spans_by_thread))]
    for r, spans in zip(report, spans_by_thread):
        r.operations = [("op", t0, t1) for t0, t1 in spans]
    return report


def test_overlap_share():
    assert T.overlap_share(span_report([[(0, 1), (2, 3)], [(4, 5), (6, 7)], [(8, 9)]])) == 0.0       # strictly sequential
    assert T.overlap_share(span_report([[(0, 1), (1.5, 2)], [(0, 1), (1.5, 2)]])) == 1.0
    assert T.overlap_share(span_report([[(0, 1), (2, 3), (4, 5), (6, 7)], [(2.5, 2.6)]])) == 0.4     # two of five
    assert T.overlap_share(span_report([[(0, 1), (0.5, 2)]])) == 0.0                                 # the same thread does not count
    assert T.overlap_share(span_report([[], []])) == 0.0
    report = T.run_threads([sleeper(index, 4, 0.03) for index in range(4)], 10)                      # barrier-started equal sleeps
    assert T.overlap_share(report) == 1.0
    assert 0.12 <= T.wall_time(report) < 4 * 4 * 0.03              # four sleeps of 0.03 s, and less than the 16 one after the other


# ------------------------------------------------------------------------------------------------ the reader worker loop

class HostTensor(list):
    def cpu(self):
        return self

    def tolist(self):
        return list(self)


class ModelReader:
    """The calls of threadrun.thread_operations on the corpus of readershapes.py, answered from readershapes.expected and
    the models after 1 ms of sleep.  `wrong`: the name of one call whose answer lacks its last element."""

    def __init__(self, e, wrong=None):
        self.e, self.wrong, self.position, self.calls = e, wrong, 0, 0

    def _answer(self, name, value):
        time.sleep(0.001)
        self.calls += 1
        return value[:-1] if name == self.wrong else value

    @staticmethod
    def _u64(values):
        return np.array(values, dtype=np.uint64)

    @staticmethod
    def _text(raw, fold):
        return (raw.lower(), R.NEEDLE.lower()) if fold else (raw, R.NEEDLE)

    def close(self):
        self.e = None

    def tell(self):
        return self.position

    def seek(self, offset):
        self.position = min(offset, self.e["size"])
        return self.position

    def read(self, n=None):
        data = self.e["raw"][self.position:] if n is None else self.e["raw"][self.position:self.position + n]
        self.position += len(data)
        return self._answer("read", data)

    def count_lines(self):
        return self._answer("count_lines", self.e["N"])

    def line_hashes(self, first=0, count=None, seed=0):
        return self._answer("line_hashes", self._u64(self.e["hashes"][seed][first:first + count]))

    def line_hashes_to_tensor(self, first=0, count=None, seed=0):
        return self._answer("line_hashes_to_tensor", HostTensor(self.e["hashes"][seed][first:first + count]))

    def field_spans(self, j, first, count, delimiter):
        spans = self.e["spans"][(j, delimiter[0])][first:first + count]
        return self._answer("field_spans", (self._u64([s for s, _ in spans]), np.array([n for _, n in spans], dtype=np.int64)))

    def read_fields(self, j, first, count):
        return self._answer("read_fields", self.e["field3"][first:first + count])

    def read_columns(self, fields, first, count):
        return self._answer("read_columns", [self.e["values"][(j, R.TAB)][first:first + count] for j in fields])

    def field_hashes(self, j, first=0, count=None, delimiter=b"\t", seed=0):
        keys = self.e["keys"][(j, delimiter[0], seed)]
        return self._answer("field_hashes", self._u64(keys if count is None else keys[first:first + count]))

    def count_by_field(self, j, first=0, count=None, delimiter=b"\t", seed=0):
        lines, counts, missing, _ = groups_of(self.e, j, delimiter[0], first, count)
        return self._answer("count_by_field", (self._u64(lines), self._u64(counts), missing))

    def value_counts(self, j, limit=None, first=0, count=None, delimiter=b"\t", seed=0):
        return self._answer("value_counts", groups_of(self.e, j, delimiter[0], first, count)[3][:limit])

    def sum_by_field(self, key, value):
        groups, missing = self.e["sums"][(key, value)]
        column = lambda name, dtype: np.array([g[name] for g in groups], dtype=dtype)          # noqa: E731
        return self._answer("sum_by_field", (column("line", np.uint64), column("count", np.uint64), column("numbers", np.uint64),
                                             [g["sum"] for g in groups], column("min", np.int64), column("max", np.int64), missing))

    def where_field(self, j, values):
        assert (j, tuple(values)) == (1, T.READER_KEYS)
        return self._answer("where_field", self._u64(self.e["selected"]))

    def first_occurrences(self, seed=0):
        return self._answer("first_occurrences", self._u64(self.e["first_occurrences"]))

    def count_distinct_lines(self, seed=0):
        return self._answer("count_distinct_lines", len(self.e["first_occurrences"]))

    def grep_regex(self, pattern, limit=None, ignore_case=False):
        numbers, lines = self.e["regex"][(pattern, ignore_case)]
        return self._answer("grep_regex", (self._u64(numbers[:limit]), lines[:limit]))

    def count_matching_lines_regex(self, pattern, ignore_case=False):
        return self._answer("count_matching_lines_regex", len(self.e["regex"][(pattern, ignore_case)][0]))

    def grep(self, pattern, start=0, end=None, ignore_case=False):
        numbers = grepgen.grep_of(*self._text(self.e["raw"], ignore_case), start, end)[0]
        return self._answer("grep", (numbers, [range_of(self.e, int(k), 1) for k in numbers]))

    def find_all(self, pattern, start=0, end=None, ignore_case=False):
        return self._answer("find_all", self._u64(grepgen.matches_of(*self._text(self.e["raw"], ignore_case), start, end)))

    def count_matches_each(self, patterns, start=0, end=None):
        return self._answer("count_matches_each", self._u64([len(grepgen.matches_of(self.e["raw"], p, start, end)) for p in patterns]))

    def find_all_any(self, patterns, start=0, end=None, limit=None):
        found = sorted((p, i) for i, x in enumerate(patterns) for p in grepgen.matches_of(self.e["raw"], x, start, end))[:limit]
        return self._answer("find_all_any", (self._u64([p for p, _ in found]), self._u64([i for _, i in found])))

    def line_numbers(self, offsets):
        return self._answer("line_numbers", grepgen.line_numbers_of(self.e["raw"], offsets))

    def line_starts(self, lines):
        return self._answer("line_starts", self._u64([self.e["starts_ext"][min(k, self.e["N"] + 1)] for k in lines]))

    def read_line_ranges(self, ranges):
        return self._answer("read_line_ranges", [range_of(self.e, first, count) for first, count in ranges])

    def read_ranges(self, ranges):
        return self._answer("read_ranges", [self.e["raw"][o:o + s] for o, s in ranges])


@pytest.fixture(scope="module")
def model_world():
    """The entries of test_gpu_reader_shapes.world that need neither the library nor the oracle."""
    return {"reader": T.plain_reader_world()}


PARALLELIZATIONS = (3, 64, 0, 5, 64, 3, 0, 1)


def model_workers(model_world, wrong=None):
    """Eight threads as test_gpu_threads.test_readers_side_by_side sets them up: readers opened and lists built here, on
    the main thread.  `wrong`: (thread, call)."""
    readers, workers = [], []
    for index, parallelization in enumerate(PARALLELIZATIONS):
        def open_model(path, _, index=index):
            return ModelReader(model_world["reader"][path], wrong[1] if wrong and wrong[0] == index else None)
        f, operations = T.thread_operations(open_model, model_world, index, parallelization, 0 if parallelization == 1 else 16, tensors=True)
        readers.append(f)
        workers.append(lambda progress, operations=operations: T.run_operations(progress, operations))
    return readers, workers


def test_worker_loop_with_a_correct_model(model_world):
    readers, workers = model_workers(model_world)
    report = T.run_threads(workers, 120)
    T.assert_clean(report)
    assert [r.result for r in report] == [25] * 7 + [9]                     # 8 of every family, 16 seeded, the whole file
    assert [f.calls >= r.result for f, r in zip(readers, report)] == [True] * 8
    assert [f.e["path"] for f in readers] == ["tail", "closed", "closed", "tail", "tail", "closed", "closed", "tail"]
    for r in report:                                                        # every thread runs every family
        labels = [label.split("(")[0] for label, _, _ in r.operations]
        assert {"count_by_field", "sum_by_field", "first_occurrences", "where_field", "read_columns", "grep_regex", "line_hashes_to_tensor",
                "seek", "read"} <= set(labels), labels
    share = T.overlap_share(report)
    print("overlap share of the model: %.2f" % share)
    assert share >= 0.5


def test_worker_loop_names_the_thread_and_operation_of_a_wrong_answer(model_world):
    _, workers = model_workers(model_world, wrong=(5, "first_occurrences"))
    report = T.run_threads(workers, 120)
    assert [r.index for r in report if r.exception is not None] == [5]
    assert isinstance(report[5].exception, T.WrongAnswer) and report[5].label == "first_occurrences()"
    assert all(r.stuck is None for r in report)
    with pytest.raises(pytest.fail.Exception) as failure:
        T.assert_clean(report)
    assert "thread 5 failed in first_occurrences()" in str(failure.value)
    assert "thread 4" not in str(failure.value) and "thread 6" not in str(failure.value)


def test_the_lists_are_seeded(model_world):
    """The same thread index gives the same list, another index another one."""
    labels = [[label for label, _, _ in T.thread_operations(lambda path, _: ModelReader(model_world["reader"][path]), model_world, index, 3, 16, tensors=True)[1]]
              for index in (0, 0, 2)]
    assert labels[0] == labels[1] and labels[0] != labels[2] and len(labels[0]) == 25
