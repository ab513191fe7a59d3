"""Callers on several threads, for test_threadrun.py (on the CPU, with stand-ins) and test_gpu_threads.py (the library).

run_threads starts every worker as a daemon thread behind one barrier and joins them all against one shared deadline;
a worker announces each operation in its Progress slot before it starts it, so that the report says for every thread what
it returned or raised, when each operation ran, and -- if the deadline passed -- in which operation it is stuck.
overlap_share says how much of that really ran side by side, assert_clean fails for every exception and ends the whole
pytest session for a stuck thread: a thread that does not come back from a GPU call means that nothing more may be
started on that GPU -- which is why close_unless_stuck, called in front of it, leaves every reader open in that case.

The second half is the reader worker loop: thread_operations opens a reader through the `open` callable it is given and
builds the thread's list of (label, call, wanted) from the seeded query_operations of test_gpu_reader_shapes.py and
test_gpu_column_shapes.py, run_operations calls and compares.  test_threadrun.py drives the same two functions with a
model reader, which is the evidence that a wrong answer on one thread fails, by thread and operation."""
import contextlib
import random
import threading
import time
import traceback

import pytest

STUCK_RETURNCODE = 3


class Progress:
    """One thread's slot: the label of the operation in progress (None between two) and the operations finished so far."""

    def __init__(self):
        self.label = None
        self.began = None
        self.failed = None
        self.operations = []             # [(label, t0, t1)] by time.monotonic()

    def begin(self, label):
        self.label, self.began = label, time.monotonic()

    def end(self):
        self.operations.append((self.label, self.began, time.monotonic()))
        self.label = None

    @contextlib.contextmanager
    def operation(self, label):
        """The first operation that raises stays in `failed`, whatever a finally clause runs after it: the report names it."""
        self.begin(label)
        try:
            yield
        except BaseException:
            if self.failed is None:
                self.failed = label
            raise
        self.end()


class ThreadReport:
    """What became of one worker: `result` or `exception` (with `trace`, its traceback text, and `label`, the operation it
    came from, or None), `operations` [(label, t0, t1)], and `stuck`: the label of the operation in progress when the
    deadline passed, None for a worker that came back."""

    def __init__(self, index):
        self.index = index
        self.result = None
        self.exception = None
        self.trace = None
        self.label = None
        self.operations = []
        self.stuck = None

    def __repr__(self):
        state = "stuck in %r" % self.stuck if self.stuck is not None else "raised %r in %r" % (self.exception, self.label) \
            if self.exception is not None else "returned"
        return "<thread %d: %s, %d operations>" % (self.index, state, len(self.operations))


BETWEEN = "(between two operations)"


def run_threads(workers, deadline_s):
    """Run every callable of `workers` on a daemon thread of its own, all released together by one barrier; each is called
    with its Progress slot.  All threads are joined against one deadline, `deadline_s` from now -- never indefinitely --
    and one ThreadReport per worker comes back, in the order of `workers`."""
    barrier = threading.Barrier(len(workers))
    slots = [Progress() for _ in workers]
    reports = [ThreadReport(index) for index in range(len(workers))]
    deadline = time.monotonic() + deadline_s

    def body(index):
        report, slot = reports[index], slots[index]
        try:
            barrier.wait(deadline_s)
            report.result = workers[index](slot)
        except BaseException as failure:             # noqa: B902 (reported, whatever it is)
            report.exception, report.trace = failure, traceback.format_exc()
            report.label = slot.failed if slot.failed is not None else slot.label

    threads = [threading.Thread(target=body, args=(index,), daemon=True, name="worker-%d" % index) for index in range(len(workers))]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join(max(0.0, deadline - time.monotonic()))
    for report, slot, thread in zip(reports, slots, threads):
        if thread.is_alive():
            report.stuck = slot.label if slot.label is not None else BETWEEN
        report.operations = list(slot.operations)
    return reports


def overlap_share(report):
    """The share of all operations whose [t0, t1] intersects an operation of another thread (0.0 for no operations)."""
    spans = [(t0, t1, r.index) for r in report for _, t0, t1 in r.operations]
    if not spans:
        return 0.0
    shared = sum(1 for t0, t1, index in spans if any(other != index and a <= t1 and t0 <= b for a, b, other in spans))
    return shared / len(spans)


def wall_time(report):
    """From the first operation's start to the last one's end, in seconds."""
    spans = [(t0, t1) for r in report for _, t0, t1 in r.operations]
    return max(t1 for _, t1 in spans) - min(t0 for t0, _ in spans) if spans else 0.0


def assert_clean(report):
    """Fail with the thread index and operation label of every exception.  A stuck thread ends the session instead
    (pytest.exit, return code 3): whatever it is stuck in still holds the GPU, and no further test may start there."""
    stuck = ["thread %d is stuck in %s" % (r.index, r.stuck) for r in report if r.stuck is not None]
    failed = ["thread %d failed in %s: %r\n%s" % (r.index, r.label if r.label is not None else BETWEEN, r.exception, r.trace)
              for r in report if r.exception is not None]
    if stuck:
        pytest.exit("; ".join(stuck) + ": the deadline passed, nothing more is started in this session"
                    + "".join("\n" + text for text in failed), returncode=STUCK_RETURNCODE)
    if failed:
        pytest.fail("\n".join(failed), pytrace=False)


def keep_forever(thing):
    """One reference to `thing` that is never given back: it is not collected, so no finaliser of it ever runs."""
    import ctypes
    ctypes.pythonapi.Py_IncRef(ctypes.py_object(thing))


def close_unless_stuck(report, closables):
    """close() every reader or Decoder of `closables` -- unless a thread of `report` is stuck (`report` None: no threads
    ran).  A stuck thread is still inside one of them, and each is used by one thread at a time; closing also synchronises
    with the GPU, which after a hang would not return and is more work started there.  They are then kept from being
    collected as well, since their finalisers close them.  For a finally clause around run_threads and assert_clean, so that
    it also runs when assert_clean ends the session -> whether they were closed."""
    if report is not None and any(r.stuck is not None for r in report):
        for thing in closables:
            keep_forever(thing)
        return False
    for thing in closables:
        thing.close()
    return True


# ------------------------------------------------------------------------------------------------ the reader worker loop

class WrongAnswer(AssertionError):
    pass


def run_operations(progress, operations):
    """Call and compare, one labelled operation after the other -> how many there were."""
    for label, call, want in operations:
        with progress.operation(label):
            got = call()
            if got != want:
                raise WrongAnswer("%s returned %.300r, wanted %.300r" % (label, got, want))
    return len(operations)


THREADS_SEED = 0x7EAD5
READER_REGEX = rb"^[0-9]+\t[a-e]*,"                  # readershapes.FIELD_REGEX
COLUMNS_REGEX = rb"^[0-9]+\tGETS?\t-"
READER_KEYS = (b"ab", b"", b"ERROR", b"error")


def variant_of(index):
    """Threads alternate between the variants; with the corpus alternating too, four threads hold the four pairs."""
    return ("tail", "closed")[(index + 1) // 2 % 2]


def extend_reader_world(e):
    """What the operations below want from the corpus of readershapes.py beyond readershapes.expected: the sums and the
    selection of the column calls, from the models of columnshapes.py.  Computed once, on the main thread."""
    import fieldmatch as FM
    import fieldnum as FN
    import readershapes as R
    e["sums"] = {(1, 0): FN.group_sums(e["raw"], R.NL, R.TAB, 1, 0)}
    e["selected"] = FM.selected(FM.flags_of(e["raw"], R.NL, R.TAB, 1, READER_KEYS, None, number=FN.number), False, 0, None, None)
    e["selected_range"] = FM.selected(FM.flags_of(e["raw"], R.NL, R.TAB, 0, None, (100, 2_000), number=FN.number), False, 0, None, None)
    assert len(e["selected"]) > 100 and len(e["selected_range"]) > 100
    return e


def plain_reader_world(variants=("tail", "closed")):
    """{variant: e} as test_gpu_reader_shapes.world builds it, without what needs the library or the oracle (the file and the
    block map; `path` is the variant's name), and extended."""
    import readershapes as R
    out = {}
    for variant in variants:
        e = dict(R.expected(variant))
        e.update(path=variant, size=len(e["raw"]), N=len(e["newlines"]), n=len(e["lines"]), starts_ext=e["line_starts"].tolist() + [len(e["raw"])])
        out[variant] = extend_reader_world(e)
    return out


def extend_columns_world(e):
    """... and from the corpus of columnshapes.py beyond columnshapes.expected: the groups, the distinct lines and the regex
    of the older calls, from the models of readershapes.py."""
    import readershapes as R
    e["groups1"] = R.groups_of(e["fields"][1])
    e["first_occurrences"] = R.first_occurrences_of(e["lines"])
    e["regex_lines"] = R.reference_regex(e["raw"], COLUMNS_REGEX)
    assert len(e["regex_lines"][0]) > 10
    return e


def held_line_hashes(f, native, first, count):
    """line_hashes as its tensor form holds it -- on the device, in the reader's context --, then the take to host memory:
    the device-resident path without torch, which cannot start in a process whose GPU this library opened first."""
    import ctypes
    import numpy as np
    lib, handle = native.lib(), f._open_reader()._h
    n = ctypes.c_uint64()
    assert lib.mi355x_bz2_reader_line_hashes(handle, 10, 0, first, count, 1, ctypes.byref(n)) == 0
    out = np.empty(n.value + 1, dtype=np.uint64)
    assert lib.mi355x_bz2_reader_take_line_hashes(handle, out.ctypes.data, n.value, 0) == 0
    return out[:n.value].tolist()


def every_family(f, e, corpus, rng, native=None, tensors=False):
    """One operation of each family that every thread runs whatever its seed draws: the three group-bys (whose sort, select
    and reduce-by-key run on the null stream that all threads share), a selection, columns, a regex, a result that stays
    on the device, and a seek with a read, which moves the position -- the only operation here that does.
    `tensors`: the device result is line_hashes_to_tensor's torch tensor -- only for a process that imported torch first,
    or a model --, else held_line_hashes."""
    from test_gpu_column_shapes import summed, summed_model
    from test_gpu_reader_shapes import grouped
    n, size, raw = e["n"], e["size"], e["raw"]
    first, count = rng.randrange(n), rng.choice([1, 5, 300])
    at, length = rng.randrange(size), rng.choice([1, 1_000, 65_536])
    moved = min(at + length, size)

    def seek_and_read():
        back = f.tell()
        got = (f.seek(at), f.read(length), f.tell())
        f.seek(back)
        return got

    def to_list(tensor):
        return tensor.cpu().tolist()

    if corpus == "reader":
        import readershapes as R
        hashes, fields = e["hashes"][0], [e["values"][(1, R.TAB)], e["values"][(3, R.TAB)]]
        families = [
            ("count_by_field(3)", lambda: grouped(f.count_by_field(3)), e["groups"][(3, R.TAB)][:3]),
            ("sum_by_field(1, 0)", lambda: summed(f.sum_by_field(1, 0)), summed_model(e, (1, 0))),
            ("first_occurrences()", lambda: f.first_occurrences().tolist(), e["first_occurrences"]),
            ("where_field(1, values=%r)" % (READER_KEYS,), lambda: f.where_field(1, values=list(READER_KEYS)).tolist(), e["selected"]),
            ("grep_regex(%r)" % READER_REGEX, lambda: (lambda got: (got[0].tolist(), got[1]))(f.grep_regex(READER_REGEX)),
             e["regex"][(READER_REGEX, False)]),
        ]
    else:
        hashes, fields = e["hashes"], [e["fields"][1], e["fields"][3]]
        families = [
            ("count_by_field(1)", lambda: grouped(f.count_by_field(1)), e["groups1"][:3]),
            ("sum_by_field(1, 2)", lambda: summed(f.sum_by_field(1, 2)), summed_model(e, (1, 2))),
            ("first_occurrences()", lambda: f.first_occurrences().tolist(), e["first_occurrences"]),
            ("where_field(1, values=[GET, GE, ''])", lambda: f.where_field(1, values=[b"GE", b"GET", b""]).tolist(),
             [k for k, flag in enumerate(e["flags"]["ge-get-empty"]) if flag]),
            ("grep_regex(%r)" % COLUMNS_REGEX, lambda: (lambda got: (got[0].tolist(), got[1]))(f.grep_regex(COLUMNS_REGEX)), e["regex_lines"]),
        ]
    return families + [
        ("read_columns([1, 3], %d, %d)" % (first, count), lambda: f.read_columns([1, 3], first, count), [c[first:first + count] for c in fields]),
        ("line_hashes_to_tensor(%d, %d)" % (first, count), lambda: to_list(f.line_hashes_to_tensor(first, count)), hashes[first:first + count])
        if tensors else
        ("line_hashes held on the device(%d, %d)" % (first, count), lambda: held_line_hashes(f, native, first, count), hashes[first:first + count]),
        ("seek(%d) + read(%d)" % (at, length), seek_and_read, (at, raw[at:at + length], moved)),
    ]


def thread_operations(open, world, index, parallelization, seeded, native=None, sample=4, tensors=False):
    """Open thread `index`'s reader -- open(path, parallelization) -- and build its list -> (reader, [(label, call, wanted)]).

    `world` is {"reader": {variant: e}, "columns": {variant: e}} with whichever corpus the thread uses: even threads the
    one of readershapes.py, odd ones the one of columnshapes.py, with the variant of variant_of.  The list is every_family in
    seeded order, mixed with `seeded` operations drawn from the corpus's query_operations (`sample` from each list built),
    and at the end the whole file by read() from offset 0, with tell() before and after.  The rng is seeded from
    (THREADS_SEED, index)."""
    corpus = ("reader", "columns")[index % 2] if "columns" in world else "reader"
    e = world[corpus][variant_of(index)]
    rng = random.Random(THREADS_SEED * 1_000 + index)
    f = open(e["path"], parallelization)
    shape = (parallelization, None, False)
    operations = every_family(f, e, corpus, rng, native, tensors)
    while len(operations) < 8 + seeded:
        if corpus == "reader":
            from test_gpu_reader_shapes import query_operations
            drawn = query_operations(f, e, shape, rng)
        else:
            from test_gpu_column_shapes import query_operations
            drawn = query_operations(f, native, e, shape, rng)
        operations += rng.sample(drawn, min(sample, 8 + seeded - len(operations)))
    rng.shuffle(operations)

    def whole_file():
        got = f.tell(), f.seek(0), f.read(), f.tell()
        f.seek(0)
        return got

    return f, operations + [("read() of the whole file", whole_file, (0, 0, e["raw"], e["size"]))]


def churn_operations(open, world, index, parallelization, rng, native=None, count=3):
    """A reader opened for one round of open, query, close -> (reader, `count` operations drawn from one query_operations
    list of its corpus); the corpus and the variant follow `index` as in thread_operations."""
    corpus = ("reader", "columns")[index % 2]
    e = world[corpus][variant_of(index)]
    f = open(e["path"], parallelization)
    shape = (parallelization, None, False)
    if corpus == "reader":
        from test_gpu_reader_shapes import query_operations
        drawn = query_operations(f, e, shape, rng)
    else:
        from test_gpu_column_shapes import query_operations
        drawn = query_operations(f, native, e, shape, rng)
    return f, rng.sample(drawn, count)
