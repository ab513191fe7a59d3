"""The conditions on the corpus of columnshapes.py that make test_gpu_column_shapes.py meaningful, checked on the CPU from
the raw bytes, the parts and the models alone: enough tiny blocks, every planted kind byte by byte on a launch boundary of
every cap it is promised for, the run of one-byte streams where it is said to lie, records of every sort, predicates that
are not trivial -- and the Python models pinned to each other at exactly the cuts the GPU tests use."""
import bz2

import pytest

import columnshapes as C
import fieldcols as FC
import fieldnum as FN
from columnshapes import NL, TAB


@pytest.fixture(scope="module", params=C.VARIANTS)
def c(request):
    return C.expected(request.param)


def line_of(c, offset):
    """(number, start, end) of the line that holds `offset`: end is its delimiter's offset, or the size."""
    raw = c["raw"]
    start = raw.rfind(b"\n", 0, offset) + 1
    end = raw.find(b"\n", offset)
    return raw.count(b"\n", 0, start), start, len(raw) if end < 0 else end


def test_deterministic_and_well_formed():
    raw, enc, parts = C.corpus("tail")
    C.corpus.cache_clear()
    assert C.corpus("tail") == (raw, enc, parts)
    closed = C.corpus("closed")[0]
    assert not raw.endswith(b"\n") and closed.endswith(b"\n") and closed[:-1] == raw[:-1]
    assert 240_000 < len(raw) < 260_000
    assert len(enc) > 100_000, "an input budget of 65 536 bytes would not be bounded residency"
    assert b"".join(parts) == raw and bz2.decompress(enc) == raw
    assert {len(p) for p in parts} == set(C.SIZES)


def test_blocks_and_streams(c):
    starts, size = c["block_starts"], len(c["raw"])
    assert 4 * 64 < len(starts) <= 400                    # about 300; at most the default batch: parallelization 0 is one launch
    assert sum(1 for p in c["parts"] if len(p) == 0) >= 20
    counts = {cap: len(C.launches_of(starts, size, cap)) for cap in (512, 64, 5, 3, 2, 1)}
    assert counts[512] == 1 and counts[64] >= 5 and counts[1] == len(starts), counts
    assert len(C.boundaries_of(starts, 64)) >= 4


def test_kinds_of_records(c):
    raw, lines, fields = c["raw"], c["lines"], c["fields"]
    n = len(lines)
    assert n == raw.count(b"\n") + (not raw.endswith(b"\n")) and n > 1_200
    keys = [key for key in fields[1] if key is not None]
    assert set(C.VOCABULARY) <= set(keys) and len(set(C.VOCABULARY)) == 40 and len(C.KEY256) == 256
    assert keys.count(b"GET") > 100 and keys.count(b"") > 10 and keys.count(C.KEY256) >= 3 and any(max(key, default=0) >= 0x80 for key in keys)
    values = [value for value in fields[2] if value is not None]
    for sort in (b"", b"-", b"+", b"1.5", b"12 "):
        assert sort in values, sort
    digits = {len(value.lstrip(b"+-")) for value in values if FN.number(value) is not None}
    assert digits == set(range(1, 19))
    assert any(len(value) == 19 and value.isdigit() for value in values) and any(value[:1] == b"+" and FN.number(value) for value in values)
    words = c["words"][2]
    assert words.count(FN.NOT_A_NUMBER) > 30 and words.count(FN.MISSING) > 30 and sum(1 for w in words if w > FN.MISSING) > 800
    assert all(word == FN.MISSING for word in c["words"][1023])
    assert sum(1 for w in c["words"][0] if w > FN.MISSING) > 1_000 and all(w <= FN.MISSING for w in c["words"][4])
    assert b"\n\n\n" in raw and lines.count(b"") > 10
    assert fields[3].count(None) > fields[2].count(None) > fields[1].count(None) > 30 and fields[0].count(None) == 0      # fewer fields
    fillers = sorted(len(filler) for filler in fields[3] if filler is not None)
    assert fillers[0] == 0 and fillers[-1] > 15_000 and fillers[-2] == 9_000 and fillers[-3] < 300        # (the last line's fills what is left)
    # field 0 and field 4 name their line
    for j in (0, 4):
        present = [value for value in fields[j] if value]
        assert len(set(present)) == len(present), j
    # the sums of BIG and NEG leave int64
    groups = {g["key"]: g for g in c["sums"][(1, 2)][0]}
    assert groups[C.BIG]["sum"] == 12 * C.NUMBER_MAX > 2**63 and groups[C.NEG]["sum"] == -12 * C.NUMBER_MAX < -2**63
    assert groups[C.BIG]["numbers"] == groups[C.BIG]["count"] == 12
    assert len(groups) >= 40 and c["sums"][(1, 2)][1] > 30 and any(g["numbers"] < g["count"] for g in groups.values())
    assert all(g["numbers"] == g["count"] for g in c["sums"][(1, 0)][0] if g["key"] in C.VOCABULARY[1:])


def test_predicates_are_not_trivial(c):
    n = len(c["lines"])
    counts = {name: sum(flags) for name, flags in c["flags"].items()}
    assert counts["never"] == 0 and counts["empty-range"] == 0
    assert 100 < counts["get"] < counts["ge-get-empty"] < n and counts["key256"] >= 3 and counts["set30"] > 100
    assert counts["small"] > 100 and counts["negative"] > 100 and counts["largest"] == 12
    assert b"GETS" not in C.SET_30 and len(set(C.SET_30)) == 30 and set(C.SET_30) < set(C.VOCABULARY)


def check_planted(c, b, kind):
    """The bytes around boundary b are those of `kind`, and the models give what the kind is planted for -> its line."""
    raw = c["raw"]
    if kind == "last-value-behind":
        assert raw[b - 1] == NL and b in c["line_starts"].tolist()
        number, start, end = line_of(c, b - 1)
    else:
        number, start, end = line_of(c, b)
    parts = raw[start:end].split(b"\t")
    assert parts[0] == b"%d" % number
    word = c["words"][2][number]
    if kind.startswith("last-value"):
        assert len(parts) == 3 and (end == b if kind == "last-value" else end == b - 1) and raw[end] == NL
        assert word == int(parts[2]) and c["fields"][3][number] is None
        return number
    assert len(parts) == 5 and parts[4] == b"end%d" % number and c["fields"][4][number] == parts[4]
    key_at = start + len(parts[0]) + 1
    value_at = key_at + len(parts[1]) + 1
    key, value = parts[1], parts[2]
    assert c["fields"][1][number] == key and c["fields"][2][number] == value
    if kind == "digits-18":
        assert len(value) == 18 and value.isdigit() and value_at + 2 <= b <= value_at + 16 and word == int(value)
    elif kind == "digits-19":
        assert len(value) == 19 and value.isdigit() and value_at + 1 <= b <= value_at + 18 and word == FN.NOT_A_NUMBER
        assert FN.number(raw[value_at:b]) is not None and FN.number(raw[b:value_at + 19]) is not None
    elif kind == "sign":
        assert len(value) == 19 and value[:1] == b"-" and value[1:].isdigit() and b == value_at + 1 and word == int(value) < -10**17
    elif kind == "sign-20":
        assert len(value) == 20 and value[:1] == b"-" and value[1:].isdigit() and value_at + 3 <= b <= value_at + 17
        assert word == FN.NOT_A_NUMBER and FN.text(value) == (20, value[:19])
    elif kind == "value-begins":
        assert b == value_at and raw[b - 1] == TAB and len(value) >= 2 and word == int(value)
    elif kind == "value-ends":
        assert b == value_at + len(value) and raw[b] == TAB and len(value) >= 2 and word == int(value)
    elif kind == "garbage":
        assert value == b"123x4" and b == value_at + 3 and word == FN.NOT_A_NUMBER and FN.number(raw[value_at:b]) == 123
    elif kind == "key":
        assert key == b"GET" and b == key_at + 2
        assert c["flags"]["get"][number] and c["flags"]["ge-get-empty"][number]
    elif kind == "key-miss":
        assert key == b"GETS" and b == key_at + 3
        assert not any(c["flags"][name][number] for name in ("get", "ge-get-empty", "set30", "key256", "never"))
    elif kind == "key-empty":
        assert key == b"" and b == key_at and raw[b - 1] == TAB == raw[b]
        assert c["flags"]["ge-get-empty"][number] and not c["flags"]["get"][number]
    else:
        raise AssertionError(kind)
    return number


@pytest.mark.parametrize("cap", C.CAPS)
def test_planted_kinds(c, cap):
    """With launches taken as consecutive groups of `cap` data blocks."""
    boundaries = set(C.boundaries_of(c["block_starts"], cap))
    targets = C.planted()[0]
    assert set(targets.values()) == set(C.KINDS) and set(targets) <= set(C.boundaries_of(c["block_starts"], 1))
    here = {}
    for b, kind in targets.items():
        number = check_planted(c, b, kind)
        if b in boundaries:
            here.setdefault(kind, []).append(number)
    if cap == 64:
        assert len(here) >= 2 and set(here) <= set(C.KINDS_AT_64) and set(C.KINDS_AT_64[:2]) <= set(here), here
    else:
        assert set(here) == set(C.KINDS), set(C.KINDS) - set(here)
    # the planted lines are different lines
    numbers = [check_planted(c, b, kind) for b, kind in targets.items()]
    assert len(set(numbers)) == len(numbers) == len(targets) >= 3 * len(C.KINDS) + 2


def test_the_run_of_one_byte_streams(c):
    raw, starts = c["raw"], c["block_starts"]
    run_at = C.planted()[1]
    assert starts[C.RUN_FIRST:C.RUN_FIRST + C.RUN_BLOCKS] == list(range(run_at, run_at + C.RUN_BLOCKS))
    assert starts[C.RUN_FIRST + C.RUN_BLOCKS] == run_at + C.RUN_BLOCKS
    assert raw[run_at - 252:run_at + 4] == C.KEY256 and raw[run_at + 4] == TAB and raw[run_at + 24] == TAB
    value = raw[run_at + 5:run_at + 24]
    assert value[:1] == b"-" and value[1:].isdigit() and len(value) == 19
    number, start, end = line_of(c, run_at)
    assert 19_000 < end - start < 21_000 and c["words"][2][number] == int(value) and c["fields"][1][number] == C.KEY256
    assert c["fields"][4][number] == b"end%d" % number and c["flags"]["key256"][number] and c["flags"]["negative"][number]
    after = raw.find(b"\t", run_at + 25)
    assert after > run_at + C.RUN_BLOCKS + 15_000 and raw.find(b"\n", run_at) > after
    for cap in C.CAPS:
        launches = C.launches_of(starts, len(raw), cap)
        assert any(run_at + 5 < lo < run_at + 24 for lo, _ in launches), "no boundary of cap %d inside the number" % cap
        if cap != 64:
            bare = [lo for lo, hi in launches if run_at + 24 < lo < end and NL not in raw[lo:hi] and TAB not in raw[lo:hi]]
            assert len(bare) >= 5, "no launches without a delimiter behind the number at cap %d" % cap
    # the neighbours are ordinary lines
    assert raw[start - 1] == NL and raw[end] == NL


@pytest.mark.parametrize("cap", (1, 2, 3, 5, 64, 512))
def test_the_models_agree_at_the_cuts(c, cap):
    """The text cut where the launches of a whole-file call meet: the stitched numbers and the assembled columns are
    those of the direct models over the whole text, so a disagreement on the GPU is the library's."""
    raw = c["raw"]
    launches = C.launches_of(c["block_starts"], len(raw), cap)
    assert launches[0][0] == 0 and launches[-1][1] == len(raw) and all(a[1] == b[0] for a, b in zip(launches, launches[1:]))
    summaries = [FN.summarise(raw[lo:hi], NL, TAB, 2, 4_096) for lo, hi in launches]
    stitched = FN.stitch(summaries, 2)
    assert stitched == FN.direct(raw, NL, TAB, 2)
    assert [word for word, _, _ in stitched] == c["words"][2]
    cuts = [lo for lo, _ in launches[1:]]
    for j in (1, 2, 3):
        data, fixups = FC.assemble(raw, cuts, NL, TAB, j)
        assert data == c["columns"][j][0], (cap, j)
        assert len(fixups) >= (cap < 512)
    n = len(c["lines"])
    first, count = n // 3, n // 2
    assert FC.assemble(raw, cuts, NL, TAB, 1, first, count)[0] == FC.column(raw, NL, TAB, 1, first, count)[0]
