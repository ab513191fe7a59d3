"""field_ints, sum_by_field / value_sums, read_columns, where_field / count_where_field / select_lines in every launch
shape: the layer of bz2_reader.cpp that cuts these calls into launches, stitches the per-launch summaries on the host
(stitchFieldNumbers, FieldSumQuery::stitch, stitchFields, stitchFieldHashes) and patches seam lines and the tail into
device memory -- over the corpus of columnshapes.py, whose 347 tiny blocks give 1, 6, 70, 116 or 347 launches per whole-file
call and whose planted numeric and keyed seams lie on the launch boundaries of every cap (test_columnshapes_corpus.py checks
that on the CPU, and pins the Python models to each other at those cuts).

The shapes are those of test_gpu_reader_shapes.py: (parallelization, MI355X_BZ2_READER_CONTEXTS or none, bounded residency
or not).  Every expected value comes from columnshapes.expected: the models fields.py, fieldnum.py, fieldcols.py,
fieldmatch.py (with fieldnum.number, never the library's parser) and the standard library, computed once per corpus variant,
shared, never changed; and from the oracle's block map."""
import ctypes
import io
import random
import time

import numpy as np
import pytest

import columnshapes as C
import fieldmatch as FM
import fieldnum as FN
import grepgen
from columnshapes import NL, TAB
from test_gpu_reader_shapes import FAILURE_SHAPES, ORDER_SHAPES, SHAPES, cap_of, open_shape, shape_id

pytestmark = pytest.mark.gpu

CASES = [(shape, variant) for shape in SHAPES for variant in C.VARIANTS if not shape[2] or variant == "tail"]


# ------------------------------------------------------------------------------------------------ the expected values

@pytest.fixture(scope="module")
def world(native, oracle, tmp_path_factory):
    """One entry per corpus variant: columnshapes.expected (shared, never changed), the file, and the oracle's map."""
    folder = tmp_path_factory.mktemp("columnshapes")
    out = {"folder": folder}
    for variant in C.VARIANTS:
        e = dict(C.expected(variant))
        path = folder / (variant + ".bz2")
        path.write_bytes(e["enc"])
        status, decoded, block_map, garbage = oracle.decode_file(e["enc"])
        assert status == 0 and decoded == e["raw"] and not garbage
        raw, starts = e["raw"], e["block_starts"]
        e.update(path=str(path), block_map=block_map, size=len(raw), N=len(e["newlines"]), n=len(e["lines"]), variant=variant,
                 starts_ext=e["line_starts"].tolist() + [len(raw)],
                 line_index={**{s: int(np.searchsorted(e["newlines"], s)) for s in starts}, len(raw): len(e["newlines"])})
        assert sorted({b for b in block_map.values()}) == starts + [len(raw)]
        # the planted lines: (line, kind, the field that names it, its value)
        e["planted"] = []
        for b, kind in sorted(C.planted()[0].items()):
            line = line_of(e, b - 1 if kind == "last-value-behind" else b)
            j = 4 if e["fields"][4][line] is not None else 0
            e["planted"].append((line, kind, j, e["fields"][j][line], b))
        e["run_line"] = line_of(e, C.planted()[1])
        e["long_filler_line"] = next(k for k, filler in enumerate(e["fields"][3]) if filler is not None and len(filler) == C.LONG_FILLER[1])
        out[variant] = e
    return out


def line_of(e, offset):
    """L(offset): the number of the line that holds it."""
    return int(np.searchsorted(e["newlines"], offset, "left"))


def seams_of(e, shape):
    """The launch boundaries of a whole-file call in this shape that the tests look at: the planted ones and a spread of
    the others (for one launch there is none: those of cap 64 stand in, as places like any other)."""
    boundaries = C.boundaries_of(e["block_starts"], min(cap_of(shape), 64))
    planted = [b for b in boundaries if b in C.planted()[0]]
    return sorted(set(planted + boundaries[::max(1, len(boundaries) // 8)]))


def windows_of(e, shape):
    """(first, count) over the numbering of field_ints: starting and ending on seam lines, one line behind a seam, the
    long line around the run of one-byte streams and its neighbours, the line with the filler of 9 000 bytes, at and past the
    end, empty, and count=10**12."""
    n = e["n"]
    lines = sorted({line_of(e, b) for b in seams_of(e, shape)})
    every = sorted({line_of(e, b) for b in C.boundaries_of(e["block_starts"], min(cap_of(shape), 64))})
    following = next(k for k in every if k > lines[1])              # from one seam line to the next one there is
    run, long_filler = e["run_line"], e["long_filler_line"]
    windows = [(lines[0], 1), (lines[1], following - lines[1] + 1), (lines[0] + 1, 5), (lines[-1] + 1, 1), (lines[-1] - 2, 4)]
    windows += [(k, 1) for k in lines[2:6]] + [(k - 1, 3) for k in lines[3:5]]
    windows += [(run, 1), (run - 1, 3), (run + 1, 2), (long_filler - 1, 3)]
    return windows + [(n - 1, 5), (n, 1), (7, 0), (0, 3), (n - 3, 10**12)]


def launches_of(e, shape):
    return len(C.launches_of(e["block_starts"], e["size"], cap_of(shape)))


def tier_of(e, shape):
    """How many whole-file passes a shape affords.  With more than 100 launches per pass (parallelization 1 and 3) only the
    first set and the first range are selected over the whole file -- select_lines and the inverted count for the set alone,
    the limits in a window --; with more than 10 (parallelization 5) every set and range is, but select_lines goes to the
    first of each and the inverted form is counted.  The rest is done in the windows.  In those two tiers the planted lines
    are asked for by their name over the whole file all at once, and one by one in windows."""
    launches = launches_of(e, shape)
    return "minimal" if launches > 100 else "reduced" if launches > 10 else "full"


# ------------------------------------------------------------------------------------------------ the call families

def ints(got):
    assert got.dtype == np.int64 and got.ndim == 1
    return got.tolist()


SUMS = {}                        # FN.group_sums of a window, computed once, shared, never changed


def group_sums(e, pair, first=0, count=None):
    if (first, count) == (0, None):
        return e["sums"][pair]
    key = (e["variant"], pair, first, count)
    if key not in SUMS:
        SUMS[key] = FN.group_sums(e["raw"], NL, TAB, pair[0], pair[1], min(first, e["n"]), count)
    return SUMS[key]


def summed(got):
    """sum_by_field's seven results as plain values."""
    lines, counts, numbers, sums, mins, maxs, missing = got
    assert lines.dtype == counts.dtype == numbers.dtype == np.uint64 and mins.dtype == maxs.dtype == np.int64
    assert isinstance(sums, list) and all(type(s) is int for s in sums) and isinstance(missing, int)
    return lines.tolist(), counts.tolist(), numbers.tolist(), sums, mins.tolist(), maxs.tolist(), missing


def summed_model(e, pair, first=0, count=None):
    groups, missing = group_sums(e, pair, first, count)
    return tuple([g[name] for g in groups] for name in ("line", "count", "numbers", "sum", "min", "max")) + (missing,)


def ranked(groups):
    order = sorted(range(len(groups)), key=lambda i: (-groups[i]["sum"], groups[i]["line"]))
    return [(groups[i]["key"], groups[i]["sum"], groups[i]["numbers"]) for i in order]


def check_ints(f, e, shape):
    for j in (0, 4, 1023):                                           # (field 2: launches_by_call)
        assert ints(f.field_ints(j)) == e["words"][j], "field_ints(%d)" % j
    want = e["words"][2]
    for first, count in windows_of(e, shape):
        assert ints(f.field_ints(2, first, count)) == want[first:first + count], "field_ints(2, %d, %d)" % (first, count)


def check_sums(f, e, shape):
    windows = windows_of(e, shape)
    assert summed(f.sum_by_field(1, 0)) == summed_model(e, (1, 0)), "sum_by_field(1, 0)"          # ((1, 2): launches_by_call)
    for pair in C.SUMS:
        for first, count in windows[:7] + windows[-7:]:
            assert summed(f.sum_by_field(pair[0], pair[1], first, count)) == summed_model(e, pair, first, count), \
                "sum_by_field(%d, %d, %d, %d)" % (pair + (first, count))
    groups = {g["key"]: g["sum"] for g in e["sums"][(1, 2)][0]}
    assert groups[C.BIG] > 2**63 and groups[C.NEG] < -2**63                      # the sums that leave int64 were compared
    assert f.value_sums(1, 2, 5) == ranked(e["sums"][(1, 2)][0])[:5], "value_sums(1, 2, 5)"
    for first, count in (windows[1], windows[-1]):
        assert f.value_sums(1, 2, None, first, count) == ranked(group_sums(e, (1, 2), first, count)[0]), \
            "value_sums(1, 2, None, %d, %d)" % (first, count)


def check_columns(f, e, shape):
    fields = e["fields"]
    assert f.read_columns([4]) == [fields[4]], "read_columns([4])"
    for first, count in windows_of(e, shape):
        assert f.read_columns([1, 3], first, count) == [fields[j][first:first + count] for j in (1, 3)], "read_columns([1, 3], %d, %d)" % (first, count)
    for line in (e["long_filler_line"], e["run_line"]):
        got = f.read_columns([3], line - 1, 3)
        assert got == [fields[3][line - 1:line + 2]] and len(got[0][1]) >= C.LONG_FILLER[1], "read_columns([3], %d, 3)" % (line - 1)


def how_of(name, **how):
    j, values, between = C.PREDICATES[name]
    return j, dict(how, values=list(values)) if values is not None else dict(how, between=between)


def agree(f, e, name, calls=("where", "count", "select"), **how):
    """where_field, count_where_field and select_lines under predicate `name` against the model's flags."""
    want = FM.selected(e["flags"][name], how.get("invert", False), how.get("first", 0), how.get("count"), how.get("limit"))
    j, arguments = how_of(name, **how)
    label = "(%d, %s, %r)" % (j, name, how)
    if "where" in calls:
        got = f.where_field(j, **arguments)
        assert got.dtype == np.uint64 and got.tolist() == want, "where_field" + label
    if "count" in calls:
        assert f.count_where_field(j, **arguments) == len(want), "count_where_field" + label
    if "select" in calls:
        numbers, lines = f.select_lines(j, **arguments)
        assert numbers.tolist() == want and lines == [e["whole_lines"][i] for i in want], "select_lines" + label
    return want


VALUE_SETS = ("get", "ge-get-empty", "key256", "set30", "never")
RANGES = ("small", "negative", "largest", "empty-range")


def check_where(f, e, shape):
    """Every set and every range, with and without invert: over the whole file as far as tier_of lets them, and all of them
    in the windows."""
    windows = windows_of(e, shape)
    tier = tier_of(e, shape)
    for names in (VALUE_SETS, RANGES):
        for k, name in enumerate(names):
            if tier == "full":
                agree(f, e, name)
                agree(f, e, name, invert=True)
            elif tier == "reduced":
                agree(f, e, name, ("where",) if k else ("where", "select"))
                agree(f, e, name, ("count",), invert=True)
            elif name == "get":
                agree(f, e, name, ("where", "select"))
                agree(f, e, name, ("count",), invert=True)
            elif k == 0:
                agree(f, e, name, ("where",))
        for k, (first, count) in enumerate(windows):
            agree(f, e, names[k % len(names)], first=first, count=count, invert=k % 3 == 2)
            # (a window with the line around the run is 90 launches at parallelization 1)
            if tier != "minimal" or not first <= e["run_line"] < first + count:
                agree(f, e, names[0], ("where", "count", "select") if tier == "full" else ("where",), first=first, count=count, invert=k % 2 == 1)
    total = sum(e["flags"]["ge-get-empty"])
    for limit in (0, 1, total - 1, total + 1):
        if tier != "minimal":
            got = agree(f, e, "ge-get-empty", ("where", "count", "select") if tier == "full" else ("where",), limit=limit)
            assert len(got) == min(limit, total)
    first = windows[1][0]
    within = sum(e["flags"]["ge-get-empty"][first:first + 300])
    assert within > 10
    for limit in (0, 1, within - 1, within + 1):
        assert len(agree(f, e, "ge-get-empty", first=first, count=300, limit=limit)) == min(limit, within)


def check_planted(f, e, shape):
    """Every planted seam line on its own: a window that consists of nothing but a patched line."""
    fields, words, planted = e["fields"], e["words"][2], e["planted"]
    run = (e["run_line"], "run", 4, fields[4][e["run_line"]], None)
    for j in (4, 0):
        named = sorted((line, value) for line, _, field, value, _ in planted + [run] if field == j)
        assert f.where_field(j, values=[value for _, value in named]).tolist() == [line for line, _ in named], "where_field(%d, all planted)" % j
    here = set(C.boundaries_of(e["block_starts"], min(cap_of(shape), 64)))
    alone = [line for line, _, _, _, b in planted if b in here]     # the seam lines of this shape: over the whole file by their name alone
    tier = tier_of(e, shape)
    alone = alone if tier == "full" else alone[:1] + alone[-1:] if tier == "reduced" else []
    for line, kind, j, value, b in planted + [run]:
        label = "%s in line %d" % (kind, line)
        if line in alone or (kind == "run" and tier != "minimal"):
            assert f.where_field(j, values=[value]).tolist() == [line], label
        assert f.where_field(j, values=[value], first=line, count=1).tolist() == [line], label
        assert f.count_where_field(j, values=[value], first=line, count=1, invert=True) == 0, label
        numbers, lines = f.select_lines(j, values=[value], first=line - 1, count=3)
        assert numbers.tolist() == [line] and lines == [e["whole_lines"][line]], label
        assert ints(f.field_ints(2, line, 1)) == [words[line]], label
        assert f.read_columns([1, 2], line, 1) == [[fields[1][line]], [fields[2][line]]], label
        for name in ("get", "ge-get-empty", "key256", "small", "negative") if tier != "minimal" or kind != "run" else ():
            want = [line] if e["flags"][name][line] else []
            field, arguments = how_of(name, first=line, count=1)
            assert f.where_field(field, **arguments).tolist() == want, (label, name)


def launches_by_call(f, e):
    """{call: launches it made}, from statistics()["batches"] before and after: whole-file calls of one pass each."""
    counts = {}
    for name, call, want in (
            ("field_ints", lambda: ints(f.field_ints(2)), e["words"][2]),
            ("sum_by_field", lambda: summed(f.sum_by_field(1, 2)), summed_model(e, (1, 2))),
            ("count_where_field(between)", lambda: f.count_where_field(2, between=C.PREDICATES["negative"][2]), sum(e["flags"]["negative"])),
            ("read_columns", lambda: f.read_columns([0, 2, 1, 2]), [e["fields"][j] for j in (0, 2, 1, 2)]),
            ("where_field(values)", lambda: f.where_field(1, values=[b"GETS", b"never"]).tolist(),
             [k for k, key in enumerate(e["fields"][1]) if key == b"GETS"])):
        before = f.statistics()["batches"]
        got = call()
        counts[name] = f.statistics()["batches"] - before
        assert got == want, name + ", whole file"
    return counts


@pytest.mark.parametrize("shape,variant", CASES, ids=lambda v: shape_id(v) if isinstance(v, tuple) else v)
def test_every_call(native, world, monkeypatch, shape, variant):
    """The time follows the launches: a whole-file pass is 347 launches at parallelization 1 (0.28 s on an MI355X, 0.8 ms per
    launch on one context), 116 at 3 (0.08 s), 70 at 5 on four contexts (0.04 s), 6 from 64 on and 1 at the default.  Measured
    once per shape, both variants and both residencies: parallelization 1 9.5 - 10.1 s, 3 2.5 - 3.2 s, 5 on four contexts
    2.2 - 2.6 s, 64 1.2 - 1.5 s, 64 on one context 1.8 - 1.9 s, the default 1.0 s.  With every set and range selected, counted
    and fetched over the whole file, inverted too, parallelization 1 took 34 s and 3 took 11 s; what was cut there is
    named at tier_of and is still done in the windows.  read_columns makes 574 launches for the 347 of a
    pass at parallelization 1 (the fix-ups of the seam lines), where_field over values a few more than a pass."""
    e = world[variant]
    began = time.time()
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        assert f.count_lines() == e["N"]
        # the shape is what it claims to be: so many launches per pass over the file, and the residency asked for
        counts = launches_by_call(f, e)
        launches = launches_of(e, shape)
        print("launches %s %s: %r of %d" % (shape_id(shape), variant, counts, launches))
        for name in ("field_ints", "sum_by_field", "count_where_field(between)"):
            assert counts[name] == launches, (name, counts, launches)
        assert counts["read_columns"] >= launches and counts["where_field(values)"] >= launches
        statistics = f.statistics()
        if shape[2]:
            assert statistics["input_resident"] == 0 and statistics["input_bytes_uploaded"] > 0
        else:
            assert statistics["input_resident"] == 1
        for check in (check_ints, check_sums, check_columns, check_where, check_planted):
            at = time.time()
            check(f, e, shape)
            print("  %s: %.2f s" % (check.__name__, time.time() - at))
        assert f.tell() == 0, "a query moved the position"
        assert f.read() == e["raw"], "read()"
    print("seconds %s %s: %.2f" % (shape_id(shape), variant, time.time() - began))


# ------------------------------------------------------------------------------------------------ call orders

ORDER_SEED = 0xC0DE7
OPERATIONS = 60


def held_ints(f, native, j, first, count, between):
    """field_ints as its tensor form holds it -- on the device --, an unrelated call, then the take (to host memory)."""
    lib, handle = native.lib(), f._open_reader()._h
    n = ctypes.c_uint64()
    assert lib.mi355x_bz2_reader_field_numbers(handle, NL, TAB, j, first, count, 1, ctypes.byref(n)) == 0
    between()
    out = np.empty(n.value + 1, dtype=np.int64)
    assert lib.mi355x_bz2_reader_take_field_numbers(handle, out.ctypes.data, n.value, 0) == 0
    return out[:n.value].tolist()


def held_columns(f, native, fields, first, count, between):
    lib, reader = native.lib(), f._open_reader()
    n, totals = reader._field_columns(fields, first, count, b"\t", b"\n")
    between()
    out = []
    for column, total in enumerate(totals):
        data, offsets, sizes = np.zeros(total, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int64)
        assert lib.mi355x_bz2_reader_take_field_column(reader._h, column, ctypes.c_void_p(data.ctypes.data) if total else None,
                                                       ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(sizes.ctypes.data) if n else None, 0) == 0
        blob, bounds = data.tobytes(), offsets.tolist()
        out.append([blob[bounds[i]:bounds[i + 1]] if size >= 0 else None for i, size in enumerate(sizes.tolist())])
    return out


def held_matches(f, native, name, between, **how):
    lib, reader = native.lib(), f._open_reader()
    j, arguments = how_of(name, **how)
    arguments = reader._where_arguments(j, arguments.get("values"), arguments.get("between"), how.get("invert", False), how.get("first", 0),
                                        how.get("count"), how.get("limit"), b"\t", b"\n", 0)
    n, _ = reader._where_field(arguments, arguments[-1], 1)
    between()
    out = np.empty(n + 1, dtype=np.uint64)
    assert lib.mi355x_bz2_reader_take_field_matches(reader._h, out.ctypes.data, n, 0) == 0
    return out[:n].tolist()


def query_operations(f, native, e, shape, rng):
    """One seeded query of every kind of test_every_call, the held forms and a few old calls: [(label, call, wanted)] with
    results as plain values."""
    raw, size, n = e["raw"], e["size"], e["n"]
    fields, words = e["fields"], e["words"]

    def window():
        return rng.choice(windows_of(e, shape)[:-1] + [(rng.randrange(n), rng.choice([0, 1, 5, 300]))])

    first, count = window()
    j = rng.choice(C.NUMBER_FIELDS)
    pair = rng.choice(C.SUMS)
    columns = rng.choice([[1, 3], [0, 2, 1, 2], [4], [2, 3, 1023]])
    name = rng.choice(VALUE_SETS + RANGES)
    invert, limit = rng.choice([False, True]), rng.choice([None, None, 0, 3])
    how = dict(first=first, count=count, invert=invert, limit=limit)
    selected = FM.selected(e["flags"][name], invert, first, count, limit)
    selected_all = FM.selected(e["flags"][name], invert, 0, None, limit)
    field, arguments = how_of(name, **how)
    _, arguments_all = how_of(name, invert=invert, limit=limit)
    at = rng.randrange(size)
    start = rng.choice(seams_of(e, shape)) - rng.randrange(3)
    hash_window = (rng.randrange(n), 40)

    def unrelated():
        """A read of another family between a hold and its take: checked as well."""
        assert f.read_ranges([(at, 700)]) == [raw[at:at + 700]]
        assert f.line_hashes(*hash_window).tolist() == e["hashes"][hash_window[0]:hash_window[0] + 40]
        assert f.grep(b"\tGETS\t", limit=2)[0].tolist() == grepgen.grep_of(raw, b"\tGETS\t", limit=2)[0].tolist()

    def column_of(k):
        return (fields[k] if k in fields else [None] * n)[first:first + count]                # no line has a field 1023

    return [
        ("field_ints(%d, %d, %d)" % (j, first, count), lambda: ints(f.field_ints(j, first, count)), words[j][first:first + count]),
        ("field_ints(2)", lambda: ints(f.field_ints(2)), words[2]),
        ("held field_ints(%d, %d, %d)" % (j, first, count), lambda: held_ints(f, native, j, first, count, unrelated), words[j][first:first + count]),
        ("sum_by_field(%d, %d, %d, %d)" % (pair + (first, count)), lambda: summed(f.sum_by_field(pair[0], pair[1], first, count)),
         summed_model(e, pair, first, count)),
        ("sum_by_field%r" % (pair,), lambda: summed(f.sum_by_field(*pair)), summed_model(e, pair)),
        ("value_sums(1, 2, 4, %d, %d)" % (first, count), lambda: f.value_sums(1, 2, 4, first, count), ranked(group_sums(e, (1, 2), first, count)[0])[:4]),
        ("read_columns(%r, %d, %d)" % (columns, first, count), lambda: f.read_columns(columns, first, count), [column_of(k) for k in columns]),
        ("read_columns([1, 2])", lambda: f.read_columns([1, 2]), [fields[1], fields[2]]),
        ("held read_columns(%r, %d, %d)" % (columns, first, count), lambda: held_columns(f, native, columns, first, count, unrelated),
         [column_of(k) for k in columns]),
        ("where_field(%s, %r)" % (name, how), lambda: f.where_field(field, **arguments).tolist(), selected),
        ("where_field(%s, invert=%r, limit=%r)" % (name, invert, limit), lambda: f.where_field(field, **arguments_all).tolist(), selected_all),
        ("held where_field(%s, %r)" % (name, how), lambda: held_matches(f, native, name, unrelated, **how), selected),
        ("count_where_field(%s, %r)" % (name, how), lambda: f.count_where_field(field, **arguments), len(selected)),
        ("select_lines(%s, %r)" % (name, how), lambda: (lambda got: (got[0].tolist(), got[1]))(f.select_lines(field, **arguments)),
         (selected, [e["whole_lines"][i] for i in selected])),
        ("grep(GET, %d, %d)" % (start, start + 3_000), lambda: (lambda got: (got[0].tolist(), got[1]))(f.grep(b"\tGET\t", max(start, 0), start + 3_000)),
         (lambda want: (want[0].tolist(), want[1]))(grepgen.grep_of(raw, b"\tGET\t", max(start, 0), start + 3_000))),
        ("field_hashes(1, %d, %d)" % (first, count), lambda: f.field_hashes(1, first, count).tolist(), e["keys"][first:first + count]),
        ("line_hashes(%d, %d)" % (first, count), lambda: f.line_hashes(first, count).tolist(), e["hashes"][first:first + count]),
    ]


@pytest.mark.parametrize("shape", ORDER_SHAPES, ids=shape_id)
def test_call_orders(native, world, monkeypatch, shape):
    """60 operations from a fixed seed on one reader: seeks and reads, which move the position; the new calls of every
    family with seeded windows, a few old ones, and the forms that hold their result on the device, taken after calls of
    other families; and the import of maps that the same reader exported."""
    e = world["tail"]
    raw, size = e["raw"], e["size"]
    rng = random.Random(ORDER_SEED)
    exported, position = None, 0
    kinds = []
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        for index in range(OPERATIONS):
            where = "seed %#x, operation %d: " % (ORDER_SEED, index)
            kind = ("read", "query")[index] if index < 2 else rng.choice(["seek", "read", "query", "query", "query", "query", "maps"])
            if kind == "seek":
                whence = rng.choice([io.SEEK_SET, io.SEEK_CUR, io.SEEK_END])
                if whence == io.SEEK_SET:
                    offset = rng.randrange(size + 1_000)
                    target = offset
                elif whence == io.SEEK_CUR:
                    offset = rng.randrange(-min(position, 100_000), 100_000)
                    target = position + offset
                else:
                    offset = -rng.randrange(size)
                    target = size + offset
                got = f.seek(offset, whence)
                position = min(target, size)
                assert got == position, where + "seek(%d, %d)" % (offset, whence)
                kind = "read"
            if kind == "read":
                n = 1 if index == 0 else rng.choice([0, 1, 7, 1_000, 65_536, 100_000])
                data = f.read(n)
                assert data == raw[position:position + n], where + "read(%d) at %d" % (n, position)
                position += len(data)
            elif kind == "query":
                label, call, want = rng.choice(query_operations(f, native, e, shape, rng))
                assert call() == want, where + label
                kinds.append(label.split("(")[0])
            elif exported is None:
                exported = (f.line_offsets(), f.block_offsets())
                assert exported[0] == e["line_index"], where + "line_offsets()"
                assert exported[1] == e["block_map"], where + "block_offsets()"
            else:
                f.set_block_offsets(exported[1])
                f.set_line_offsets(exported[0])
                exported = None
            assert f.tell() == position, where + "tell() after " + kind
        assert index == OPERATIONS - 1
    # the seed reaches every family, a held form and an old call
    assert {"field_ints", "sum_by_field", "value_sums", "read_columns", "where_field", "count_where_field", "select_lines", "held field_ints",
            "held read_columns", "held where_field", "grep", "line_hashes"} <= set(kinds), sorted(set(kinds))


# ------------------------------------------------------------------------------------------------ failures

def bits_of(e, block):
    """(bit offset, bit offset of what follows) of data block `block`."""
    items = sorted(e["block_map"].items())
    data = [(bits, next_bits) for (bits, start), (next_bits, stop) in zip(items, items[1:]) if stop > start]
    assert len(data) == len(e["block_starts"])
    return data[block]


def families(f, e, first, count):
    """One call of each family over a window -> plain values; and what the models say."""
    got = (ints(f.field_ints(2, first, count)), summed(f.sum_by_field(1, 2, first, count)), f.value_sums(1, 2, None, first, count),
           f.read_columns([1, 3], first, count), f.where_field(1, values=[b"GET", b""], first=first, count=count).tolist(),
           f.where_field(2, between=(-5, 10**17), first=first, count=count).tolist(),
           f.count_where_field(1, values=[b"GET"], first=first, count=count, invert=True),
           (lambda numbers, lines: (numbers.tolist(), lines))(*f.select_lines(1, values=[b"GET"], first=first, count=count)))
    return got


def families_model(e, first, count):
    get = FM.selected(e["flags"]["get"], False, first, count)
    return (e["words"][2][first:first + count], summed_model(e, (1, 2), first, count), ranked(group_sums(e, (1, 2), first, count)[0]),
            [e["fields"][j][first:first + count] for j in (1, 3)],
            [i for i in range(first, first + count) if e["fields"][1][i] in (b"GET", b"")],
            FM.selected(e["flags"]["small"], False, first, count),
            len(FM.selected(e["flags"]["get"], True, first, count)), (get, [e["whole_lines"][i] for i in get]))


def failing_calls(f, first, count):
    """[(name, call)] of every family over lines [first, first + count) (None, None: the whole file)."""
    window = {} if first is None else dict(first=first, count=count)
    tag = "()" if first is None else "(%d, %d)" % (first, count)
    positional = (0, None) if first is None else (first, count)
    return [("field_ints" + tag, lambda: f.field_ints(2, *positional)), ("sum_by_field" + tag, lambda: f.sum_by_field(1, 2, *positional)),
            ("value_sums" + tag, lambda: f.value_sums(1, 2, 3, *positional)), ("read_columns" + tag, lambda: f.read_columns([1, 3], *positional)),
            ("where_field(values)" + tag, lambda: f.where_field(1, values=[b"GET"], **window)),
            ("where_field(between)" + tag, lambda: f.where_field(2, between=(0, 5), **window)),
            ("count_where_field" + tag, lambda: f.count_where_field(1, values=[b"GET"], invert=True, **window)),
            ("select_lines" + tag, lambda: f.select_lines(1, values=[b"PUT"], **window))]


@pytest.mark.parametrize("shape", FAILURE_SHAPES, ids=shape_id)
def test_damaged_block(native, world, monkeypatch, tmp_path, shape):
    """One byte flipped in the middle of a block, both true indexes imported: every family serves what keeps clear of the
    block and fails, with the status and the bit offset of a plain read, for what needs it -- and goes on serving
    afterwards.  A window whose first line begins in the good block in front of the window's first block is served too:
    its seam fix-up needs good blocks only."""
    e = world["tail"]
    blocks = C.data_blocks(e)
    d = C.block_for_damage(e)
    start, stop, _ = blocks[d]
    bits, next_bits = bits_of(e, d)
    damaged = bytearray(e["enc"])
    damaged[(bits + next_bits) // 16] ^= 0xFF
    bad = tmp_path / "damaged.bz2"
    bad.write_bytes(bytes(damaged))
    with open_shape(native, monkeypatch, str(bad), shape) as f:
        with pytest.raises(native.Bz2Error) as failure:
            f.read()
        status = failure.value.status
        assert status != 0
    in_front, behind = line_of(e, start) - 9, line_of(e, stop) + 2           # windows of 6 lines clear of the block
    inside = line_of(e, start) + 2
    assert e["starts_ext"][in_front + 6] <= start and e["starts_ext"][behind] >= stop
    # the lines across the boundaries in front of block d - 1 and of block d + 2: they begin in one good block and end in the next
    across_front, across_behind = line_of(e, blocks[d - 1][0]), line_of(e, blocks[d + 2][0])
    assert e["starts_ext"][across_front] < blocks[d - 1][0] and e["starts_ext"][across_front + 3] <= start
    assert stop < e["starts_ext"][across_behind] < blocks[d + 2][0] < e["starts_ext"][across_behind + 1] <= blocks[d + 2][1]
    with open_shape(native, monkeypatch, str(bad), shape) as f:
        f.set_block_offsets(e["block_map"])
        f.set_line_offsets(e["line_index"])
        clean = {first: families_model(e, first, 6) for first in (in_front, behind)}
        for first in (in_front, behind):
            assert families(f, e, first, 6) == clean[first], first
        failing = failing_calls(f, None, None) + failing_calls(f, inside, 2) + failing_calls(f, in_front, behind - in_front)
        for k, (name, call) in enumerate(failing):
            with pytest.raises(native.Bz2Error) as failure:
                call()
            assert failure.value.status == status, name
            assert f"bit offset {bits}" in str(failure.value), name
            # after each failure a clean call of each family is answered correctly
            first = (in_front, behind)[k % 2]
            assert families(f, e, first, 6) == clean[first], "behind the failure of " + name
        for first, count in ((across_front, 3), (across_front, 1), (across_behind, 3), (across_behind, 1)):
            assert families(f, e, first, count) == families_model(e, first, count), (first, count)
        assert f.tell() == 0 and f.read_ranges([(0, 1000), (stop, 700)]) == [e["raw"][:1000], e["raw"][stop:stop + 700]]


@pytest.mark.parametrize("shape", FAILURE_SHAPES, ids=shape_id)
def test_lying_line_index(native, world, monkeypatch, shape):
    """The imported line index gives block b one delimiter more and block b + 1 one fewer: every family fails for a window
    that needs block b, with status 106, and says which block, what was promised and what was counted; a window clear of
    both blocks is served, and so is everything once the true index is back."""
    e = world["tail"]
    blocks = C.data_blocks(e)
    b = C.block_for_lie(e)
    start, following, held = blocks[b][0], blocks[b + 1][0], blocks[b][2]
    true_index = e["line_index"]
    lying = dict(true_index)
    lying[following] += 1
    failing = (true_index[start] + 3, 3)                                       # lines that lie inside block b
    clear = (true_index[blocks[b - 1][0]] + 2, 3)                              # ... inside block b - 1
    assert true_index[following] - true_index[start] == held and failing[0] + failing[1] < true_index[following] - 1
    message = "decoded offset %d %d delimiters, it holds %d" % (start, held + 1, held)
    with open_shape(native, monkeypatch, e["path"], shape) as f:
        f.set_block_offsets(e["block_map"])
        f.set_line_offsets(lying)
        for name, call in failing_calls(f, *failing):
            with pytest.raises(native.Bz2Error) as failure:
                call()
            assert failure.value.status == 106 and "line index" in str(failure.value), name
            assert message in str(failure.value), (name, str(failure.value))
            assert families(f, e, *clear) == families_model(e, *clear), "clear of the lie, behind the failure of " + name
        f.set_line_offsets(true_index)
        assert families(f, e, *failing) == families_model(e, *failing)
        assert ints(f.field_ints(2)) == e["words"][2] and f.read_columns([1]) == [e["fields"][1]]
        assert f.tell() == 0 and f.read(1000) == e["raw"][:1000]
