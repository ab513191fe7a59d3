"""CPU suite: the crafted symbol streams of tests/crafted_symbols.py.  For every case the plain model (bz2parse.unmtf +
crafted.model_decode), the oracle, CPython's bz2 and the recorded answer of the real reference
(tests/golden/crafted_symbols_vectors.json, written by tests/golden/make_golden_symbols.py from oracle/_ref/ref_bz2 probe)
agree, and the restated planners show the branch the case is there for.  The GPU side of the same cases is
tests/test_gpu_symbol_stages.py."""
import bz2
import collections
import hashlib
import json
import os
import re

import pytest

from conftest import ROOT
import bz2enc
import bz2parse
import crafted
import crafted_symbols as cs
from test_oracle import fnv64

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "crafted_symbols_vectors.json")
GOLDEN = json.load(open(GOLDEN_PATH))
PLANNED = [name for name in cs.SCAN_NAMES if name != "full-18001"]      # the planners take a stream bit by bit
JUMPS = [f"jump-{k}" for k in range(15)]


def _constant(text, name):
    return int(re.search(r"constexpr uint32_t %s = (\d+)" % name, text).group(1))


def test_restated_constants_are_the_kernels():
    """The planners of crafted_symbols.py restate these: a changed constant fails here, not by a branch silently left
    unreached."""
    src = os.path.join(ROOT, "indexed_bzip2_amd", "csrc")
    hscan = open(os.path.join(src, "bz2_hscan.hip.h")).read()
    stage1 = open(os.path.join(src, "bz2_stage1.hip.h")).read()
    kernels = open(os.path.join(src, "bz2_kernels.hip.h")).read()
    device = open(os.path.join(src, "bz2_device.hip")).read()
    for name in ("SCAN_MAX_SPAN", "SCAN_RING_ENTRIES", "GROUP_SYMS", "MAX_SCAN_GROUPS", "SCAN_LUT_BITS"):
        assert _constant(hscan, name) == getattr(cs, name), name
    assert "SPEC_REACH = 32 * SpecShared<K>::RING - 4700" in hscan and "RING = K > 8 ? 2 * SCAN_RING_ENTRIES : SCAN_RING_ENTRIES" in hscan
    assert "( SCAN_MAX_SPAN - 24 ) / need" in hscan and "est + ( est >> 3 ) + 16" in hscan
    sym_groups = int(re.search(r"SYM_GROUPS = (\d+)", device).group(1))
    assert _constant(hscan, "SYM_CHUNKS") * sym_groups == cs.SYM_GROUPS_PER_WORKGROUP and "HSYM( SYM_GROUPS )" in device
    assert _constant(stage1, "MTF_SMALL_STRIDE") - 16 == cs.MTF_SMALL_ENTRIES
    assert _constant(kernels, "MAX_N") == cs.MAX_N


def test_encoder_entry_writes_what_it_is_given():
    """encode_block_from_symbols against the plain parser: symbols, tables, the header's selectors (surplus included), and
    the group starts it reports."""
    for name in ("selectors-rounds", "six-tables", "count-129", "jump-3"):
        c, m = cs.case(name), cs.model(name)
        block = bz2parse.parse_block(m.stream, 32)
        assert block["symbols"] == c["symbols"] and block["lengths"] == c["tables"] and block["used"] == c["declared"]
        assert block["selectors"] == c["selectors_written"] and block["n_selectors"] == len(c["selectors_written"])
        assert (block["crc"], block["orig_ptr"]) == (m.crc, m.orig_ptr)
        assert m.group_starts[0] == 32 + block["header_bits"] and len(m.group_starts) == len(c["selectors"])
        # every group start by the code lengths in front of it
        pos = m.group_starts[0]
        for g, t in enumerate(c["selectors"]):
            assert m.group_starts[g] == pos, (name, g)
            pos += sum(c["tables"][t][s] for s in c["symbols"][g * 50:(g + 1) * 50])
        assert pos == block["end_bit"]
    # encode_block_from_bwt is a caller of it (test_encode_block_streams_are_unchanged pins its streams)
    last, orig_ptr = bz2enc.bwt(b"abracadabra" * 30)
    used, symbols = bz2enc.mtf_rle2(last)
    lengths = bz2enc.skewed_lengths(len(used) + 2, sorted(range(len(used) + 2), key=lambda s: -symbols.count(s)))
    n_sel = -(-len(symbols) // 50)
    direct = bz2enc.encode_block_from_symbols(symbols, used, orig_ptr, 123, [lengths, lengths], [g % 2 for g in range(n_sel)])
    assert direct[0] == bz2enc.encode_block_from_bwt(last, orig_ptr, 123)


@pytest.mark.parametrize("name", cs.NAMES)
def test_model_oracle_and_libbz2_agree(oracle, name):
    m = cs.model(name)
    c = cs.case(name)
    assert all(s >= 2 for s in m.symbols) or name in cs.MTF_NAMES          # scan cases: literals only, a trivial column
    assert len(m.column) <= cs.MAX_N and 0 <= m.orig_ptr < len(m.column)
    d, payload, lcol, rle = oracle.decode_block(m.stream, 32, want_stages=True)
    assert (d["status"], d["bwt_length"], d["orig_ptr"], d["header_crc"], d["computed_crc"], d["decoded_size"]) == \
           (0, len(m.column), m.orig_ptr, m.crc, m.crc, len(m.out)), d
    assert d["n_symbols"] == len(m.symbols)
    assert 0 <= len(m.stream) * 8 - 32 - d["encoded_size_bits"] - 80 < 8
    assert lcol == m.column and rle == m.pre and payload == m.out
    assert bz2.decompress(m.stream) == m.out
    assert len(m.group_starts) == len(c["selectors"]) <= len(m.selectors_written)


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_reference_answers(oracle, name, tmp_path):
    """What the real reference said about the very same stream (recorded), against the oracle and the model; and against
    the reference itself where its binary is present."""
    gold = GOLDEN["cases"][name]
    m = cs.model(name)
    assert hashlib.sha256(m.stream).hexdigest() == gold["enc_sha256"], "builder drifted: rerun tests/golden/make_golden_symbols.py"
    assert gold["verdict"] == "OK"
    d, payload = oracle.decode_block(m.stream, 32)
    assert (d["status"], d["encoded_size_bits"], d["header_crc"], d["computed_crc"], d["decoded_size"], fnv64(payload)) == \
           (0, gold["size"], gold["header_crc"], gold["calc_crc"], gold["decoded"], gold["fnv64"])
    assert (m.crc, len(m.out), fnv64(m.out)) == (gold["calc_crc"], gold["decoded"], gold["fnv64"])
    if oracle.ref_available():
        p = tmp_path / "case.bz2"
        p.write_bytes(m.stream)
        assert crafted.parse_probe(oracle.ref_run("probe", p, 32)) == {k: v for k, v in gold.items() if k != "enc_sha256"}


def _plans(name):
    si = cs.scan_input(name)
    return si, cs.hscan_plan(si), {K: cs.spec_plan(si, K) for K in (4, 8)}


@pytest.mark.parametrize("name", PLANNED)
def test_scan_case_reaches_its_branch(name):
    """Conditions, not measurements: what each case must show, by the restated loops of k_hscan<1> and k_hscan_spec<4/8>,
    for the branch it is there for.  If one fails after a constant changed in bz2_hscan.hip.h, the case list is stale."""
    si, (h1, instances, left_at), spec = _plans(name)
    c = cs.case(name)
    groups = len(si.glen)
    assert h1["groups"] == groups
    if name == "long-1000":
        # the format's longest group: always the full span; k_hsym's lanes take 20 bits per symbol.  In k_hscan_spec a table
        # whose groups take 1 000 bits never passes `widthV + need + 24 <= SCAN_MAX_SPAN` (need = 1 141): every unit is a
        # full one, it is the span term that cuts, and SPEC_REACH is reached by long-800 below
        assert set(si.glen[:-1]) == {20 * 50} and groups == 71 and set(instances) == {cs.SCAN_ROWS}
        assert h1["refills"] >= 70 * 1000 // 2048
        for K in (4, 8):
            assert spec[K]["cut-span"] == 70 and spec[K]["full-units"] == groups and spec[K]["cut-reach"] == 0
    elif name == "long-800":
        # 800 bits: need = 916 leaves room for windows, five groups reach 4 x 802 > SPEC_REACH; two refills in one unit
        assert set(si.glen[:-1]) == {800}
        assert spec[8]["cut-reach"] >= 1 and spec[8]["n=5"] >= 1 and spec[8]["most-refills-at-once"] == 2
        # four waves: see test_reach_cannot_cut_a_unit_of_four
        assert spec[4]["cut-reach"] == 0 and spec[4]["n=4"] >= 1 and spec[4]["most-refills-at-once"] == 2
    elif name == "all-ones":
        assert c["tables"][0][20] == 1 and c["tables"][0][19] == 20 and set(c["symbols"][:-1]) == {19}
        assert bz2enc.canonical_codes(c["tables"][0])[19] == 0xFFFFF
        for events in (h1, spec[4], spec[8]):
            assert events["pending-over-half-in-mid-block-full-span"] >= 60
    elif name == "short-50":
        assert set(si.glen[:-1]) == {50} and groups == 201
        assert h1["m=13"] >= 1 and (cs.SCAN_MAX_SPAN - 24) // (50 + 6 + 16) == 13
        for K in (4, 8):
            assert spec[K]["step-lo-floor"] >= 1 and spec[K][f"n={K}"] >= 1
    elif name.startswith("jump-"):
        k = int(name[5:])
        assert si.glen == (50,) * k + (1000, 0)
        if k >= 1:
            # the long group leaves the span of the build it is met in, at chase index k - 1 (the first group is measured alone,
            # the next build takes up to 13); then, first of a build, it leaves that too and gets the full span
            assert left_at[0] == 1 and h1["full-after-leaving"] == 1 and sum(left_at.values()) == (2 if 2 <= k <= 13 else 1)
            assert k > 13 or k == 1 or left_at[k - 1] == 1
            for K in (4, 8):
                assert spec[K]["chain-0xffff-at-slot-0"] == 1 and spec[K]["full-after-0xffff"] == 1
    elif name == "staircase":
        assert set(si.sel[:groups - 1]) == {0, 1} and all(a != b for a, b in zip(si.sel, si.sel[1:groups - 1]))
        assert min(si.glen[:-1]) == 50 and max(si.glen) == 1000
        assert set(instances) == cs.selectable_instances()
        for K in (4, 8):
            assert spec[K]["chain-stray"] >= 1 and spec[K]["step-lo-floor"] >= 1
    elif name == "six-tables":
        assert len(c["tables"]) == 6 and len({tuple(t) for t in c["tables"]}) == 6 and h1["first-of-table"] == 6
        assert si.sel[:56] == tuple((5 * g + 1) % 6 for g in range(56))
        assert len(set(si.sel[56:72])) == 1 and len(set(si.sel[120:136])) == 1         # runs across 63/64 and 127/128
        assert h1["run-clamped-at-window"] >= 2
        for K in (4, 8):
            assert spec[K]["from-next-window"] >= 1 and spec[K]["chain-stray"] >= 1 and spec[K]["cut-table-not-seen"] == 6
    elif name.startswith("groups-"):
        want = int(name[7:])
        tail = "tail-empty" if want % 64 == 0 else "tail-partial"
        assert groups == want
        for events in (h1, spec[4], spec[8]):
            assert events[tail] == 1 and events["window-written"] == want // 64
    elif name == "eob-alone-3200":
        assert len(c["symbols"]) == 3201 and groups == 65 and si.glen[-1] == 0
        for events in (h1, spec[4], spec[8]):
            assert events["tail-partial"] == 1 and events["window-written"] == 1
    elif name == "eob-last-3199":
        assert len(c["symbols"]) == 3200 and groups == 64 and si.glen[-1] > 0
        for events in (h1, spec[4], spec[8]):
            assert events["tail-empty"] == 1
    elif name == "lut-edge":
        for t, lengths in enumerate(c["tables"]):
            used = collections.Counter(lengths[s] for g, sel in enumerate(c["selectors"]) if sel == t
                                       for s in c["symbols"][g * 50:(g + 1) * 50] if s != 20)
            assert used[cs.SCAN_LUT_BITS] >= 100 and used[cs.SCAN_LUT_BITS + 1] >= 100, (t, used)
    elif name == "selectors-rounds":
        rounds, short_take, carries, bits = cs.selector_plan(name)
        assert rounds >= 3 and short_take and carries >= {1, 2, 3, 4, 5} and bits > 2048
        assert groups == 71 and si.n_sel == 71 + 2600 and len(c["tables"]) == 6
    elif name.startswith("sym-chunks-"):
        assert groups == int(name[11:]) and groups - cs.SYM_GROUPS_PER_WORKGROUP in (-1, 0, 1)
        assert spec[8]["from-next-window"] >= 1 and spec[4]["from-next-window"] >= 1
    else:
        raise AssertionError(f"no condition written for {name}")


def test_jumps_leave_the_span_at_every_chase_index():
    """A build of k_hscan<1> chases up to 13 groups of 50 bits: the jump cases leave it at every index 0 .. 12; in
    k_hscan_spec the long group is met at slot 0 (0xFFFF, forceFull) and at a later slot."""
    left = collections.Counter()
    spec = {4: collections.Counter(), 8: collections.Counter()}
    for name in JUMPS:
        si, (h1, instances, left_at), plans = _plans(name)
        left.update(left_at)
        for K in (4, 8):
            spec[K].update(plans[K])
    assert set(left) == set(range(13))
    for K in (4, 8):
        assert spec[K]["chain-0xffff-at-slot-0"] == 14 and spec[K]["chain-0xffff-later"] >= 5


def test_reach_cannot_cut_a_unit_of_four():
    """`accHi <= SPEC_REACH` in k_hscan_spec<4>: slot 3 sees accHi = stepHi_0 + stepHi_1 + stepHi_2 with stepHi = mid + slack.
    Every usable slot passed `widthV + need + 24 <= SCAN_MAX_SPAN` with need = est + est / 8 + 16 >= 72 and mid <= est
    (est is the decayed maximum, mid a mean of the same lengths), so mid <= 875; slot 3's width is 2 (slack_0 + slack_1 +
    slack_2) <= 1024 - 24 - 72.  The sum stays below SPEC_REACH: the term can only cut units of eight (long-800)."""
    largest_est = max(est for est in range(50, 1001) if est + (est >> 3) + 16 + 24 <= cs.SCAN_MAX_SPAN)
    slack_sum = (cs.SCAN_MAX_SPAN - 24 - 72) // 2
    assert largest_est == 875 and 3 * largest_est + slack_sum < cs.SPEC_REACH
    assert 7 * largest_est > cs.SPEC_REACH


def test_full_block():
    c, m = cs.case("full-18001"), cs.model("full-18001")
    assert len(m.column) == cs.MAX_N and len(c["selectors"]) == 18001 == cs.MAX_SCAN_GROUPS - 1 and len(c["tables"]) == 6
    assert len(m.group_starts) == 18001


@pytest.mark.parametrize("name", cs.MTF_NAMES)
def test_mtf_case_reaches_its_branch(name):
    """The same for k_mtf, by its chunk rule and ByteSink restated, at every lane count a block of the case can get."""
    c = cs.case(name)
    symbols = c["symbols"][:-1]
    nd = len(c["declared"])
    lane_counts = (256, 512, 1024) if nd <= cs.MTF_SMALL_ENTRIES else (256, 512)
    assert {cs.mtf_lanes(nd, n, narrow) for n in (1, 65) for narrow in (False, True)} == set(lane_counts)
    plans = {lanes: cs.mtf_plan(symbols, lanes) for lanes in lane_counts}
    sequences = [len(d) for d in re.findall(r"d+", "".join("d" if s <= 1 else "l" for s in symbols))]
    positions = {s - 1 for s in symbols if s >= 2}
    kind = name.split("@")[0]
    for lanes, (events, alignments) in plans.items():
        assert events["bytes"] == len(cs.model(name).column)
        if kind == "digits-across-chunks":
            assert 250 <= len(symbols) <= 320
            assert set(sequences) >= set(range(1, 18)) | {19 if nd == 19 else 18} and sum(sequences) > len(symbols) * 0.8
            assert events["pushed-chunks"] >= 1 and events["empty-chunks"] >= 1 and events["same-begin"] >= 1
        elif kind == "runs-at-every-alignment":
            assert alignments >= {(a, count) for a in range(16) for count in range(1, 41)}
            assert all(events[branch] >= 1 for branch in cs.FILL_BRANCHES), events
            assert events["head-shared-with-previous-lane"] >= 1 and events["tail-shared-with-next-lane"] >= 1
        elif kind == "run-first":
            assert symbols[0] <= 1 and events["empty-chunks"] >= 1
        elif kind == "run-900000":
            assert all(s <= 1 for s in symbols) and bz2parse.zero_runs(symbols + [2]) == [cs.MAX_N]
            assert events["chunk-is-one-run"] == 1 and events["empty-chunks"] == lanes - 1 and events["run-ends-at-max-n"] == 1
        elif kind == "run-899999-literal":
            assert bz2parse.zero_runs(symbols) == [cs.MAX_N - 1] and symbols[-1] == nd
            assert events["literal-at-the-last-byte"] == 1
        elif kind == "deep-positions":
            edges = {p for e in range(15, nd, 16) for p in (e, e + 1, e + 2) if p < nd}
            assert positions >= edges and nd - 1 in positions and symbols.count(nd) >= 300
            assert (nd - 1) >> 4 == (1 if nd == 19 else 12)
        elif kind in ("count-128", "count-129"):
            assert nd == int(kind[6:]) and nd - 1 in positions
            assert (cs.mtf_lanes(128, 1), cs.mtf_lanes(129, 1)) == (1024, 512)
            assert events["pushed-chunks"] >= 1
        else:
            raise AssertionError(f"no condition written for {name}")


def test_digit_sequences_of_every_length():
    found = set()
    for nd in (19, 200):
        symbols = cs.case(f"digits-across-chunks@{nd}")["symbols"]
        found |= {len(d) for d in re.findall(r"d+", "".join("d" if s <= 1 else "l" for s in symbols))}
    assert found >= set(range(1, 20))


def test_case_list_covers_the_edges():
    names = set(cs.NAMES)
    assert names >= {"long-1000", "long-800", "all-ones", "short-50", "staircase", "six-tables", "eob-alone-3200",
                     "eob-last-3199", "lut-edge", "selectors-rounds", "full-18001", "count-128", "count-129"}
    assert names >= set(JUMPS)
    assert names >= {f"groups-{g}" for g in (63, 64, 65, 128)} | {f"sym-chunks-{g}" for g in (1023, 1024, 1025)}
    for kind in ("digits-across-chunks", "runs-at-every-alignment", "run-first", "run-900000", "run-899999-literal",
                 "deep-positions"):
        assert {f"{kind}@19", f"{kind}@200"} <= names, kind
    assert len(cs.case("count-128")["declared"]) == cs.MTF_SMALL_ENTRIES == len(cs.case("count-129")["declared"]) - 1
    assert set(GOLDEN["cases"]) == names
    # all cases but the full block and the two long runs stay below 60 000 symbols; those three kinds alone are left out of the batch
    big = {name for name in names if len(cs.case(name)["symbols"]) >= 60_000}
    assert big == {"full-18001"}
    assert {name.split("@")[0] for name in cs.big_names()} == {"full-18001", "run-900000", "run-899999-literal",
                                                              "digits-across-chunks"}


def test_symbol_batch(oracle):
    """The large batch of the GPU test, on the CPU: more than 64 and at most 640 entries (512 lanes per block in k_mtf), every
    small case at least twice, every offset a block of its case."""
    data, entries = cs.symbol_batch()
    assert 65 <= len(entries) <= 640 and cs.mtf_lanes(19, len(entries)) == 512 and cs.mtf_lanes(200, len(entries)) == 512
    assert sorted({o for _, o in entries}) == oracle.find_magic(data)
    assert collections.Counter(name for name, _ in entries) == {name: 2 for name in cs.small_names()}
    for name, off in dict(entries).items():
        d, payload = oracle.decode_block(data, off)
        assert d["status"] == 0 and payload == cs.model(name).out, name
