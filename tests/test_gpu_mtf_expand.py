"""GPU suite: k_mtf's pass B (bz2_stage1.hip.h) -- the data-parallel form, a wave per chunk (mtf_expand_chunks), and the
serial form it falls back to -- on crafted symbol streams, against the plain model of tests/crafted_symbols.py and the oracle.

Contexts keep their stages and are made under {}, MI355X_BZ2_MTF_NARROW=1 (256 lanes per block) and MI355X_BZ2_MTF_SERIAL=1
(every block through the serial pass).  Valid cases are checked three ways: the column (debug stage 0) against the model, the
record against the oracle, the payload against the model.
  (a) every MTF case of crafted_symbols under MI355X_BZ2_MTF_SERIAL=1, alone and in symbol_batch(): the serial pass would
      otherwise see damaged blocks only;
  (b) new small cases, each with 19 and with 200 declared values (k_mtf<144> and <272>), alone and all together in one
      batch of more than 64 entries (512 lanes, both instances side by side);
  (c) blocks that must take the fallback: status and record as the oracle's, the same with and without the switch.

Run on the GPU box: python -m pytest tests/test_gpu_mtf_expand.py -m gpu -q --durations=0
"""
import collections
import functools

import numpy as np
import pytest

import bz2enc
import bz2parse
import crafted
import crafted_symbols as cs
from test_gpu_decode_stages import RECORD_KEYS, check_batch, check_record, first_difference
from test_gpu_symbol_stages import check_case, check_scan_stages

pytestmark = pytest.mark.gpu

VARIANTS = {
    "wide": {},
    "mtf-256": {"MI355X_BZ2_MTF_NARROW": "1"},
    "serial": {"MI355X_BZ2_MTF_SERIAL": "1"},
}
SWITCHES = ("MI355X_BZ2_SCAN_WAVES", "MI355X_BZ2_MTF_NARROW", "MI355X_BZ2_MTF_SERIAL")
MAX_N = cs.MAX_N
WINDOW = 1024       # MTF_WINDOW of bz2_stage1.hip.h: bytes of the column a wave puts together at a time


def _set(mp, variant):
    for key in SWITCHES:
        mp.delenv(key, raising=False)
    for key, value in VARIANTS[variant].items():
        mp.setenv(key, value)


def _context(native, variant):
    with pytest.MonkeyPatch.context() as mp:
        _set(mp, variant)
        d = native.Decoder(flags=native.Decoder.KEEP_STAGES)
        d.keeps_stages = True
        d.variant = variant
        yield d
        d.close()


@pytest.fixture(scope="module", params=list(VARIANTS))
def dec(native, request):
    yield from _context(native, request.param)


@pytest.fixture(scope="module")
def serial_dec(native):
    yield from _context(native, "serial")


@pytest.fixture
def switches(dec, monkeypatch):
    _set(monkeypatch, dec.variant)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the existing cases through the serial pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cs.MTF_NAMES)
def test_existing_case_serial(native, oracle, serial_dec, monkeypatch, name):
    _set(monkeypatch, "serial")
    check_case(name, native, oracle, serial_dec)


def test_existing_batch_serial(native, oracle, serial_dec, monkeypatch):
    _set(monkeypatch, "serial")
    data, entries = cs.symbol_batch()
    want = {o: (name, cs.model(name).out, cs.model(name).crc) for name, o in entries}
    check_batch(oracle, serial_dec, data, [o for _, o in entries], want)
    for k, (name, o) in enumerate(entries):
        if name in cs.MTF_NAMES:
            lanes = cs.mtf_lanes(len(cs.model(name).declared), len(entries))
            check_scan_stages(name, serial_dec, k, o - 32, len(data) * 8, lanes)


# ---------------------------------------------------------------------------------------------------------------------
# (b) new cases
# ---------------------------------------------------------------------------------------------------------------------
def _literals(nd, count, start=0):
    """`count` literals that keep the list moving: positions 1 .. nd - 1 in a pattern without a period of 8 or 16."""
    return [2 + (start + 7 * k + k // 5) % (nd - 1) for k in range(count)]


def _new_cases():
    cases = {}
    for nd in (19, 200):
        tag = f"@{nd}"
        for n in (1, 2, 255, 256, 257):
            # empty chunks, one symbol per chunk; every third symbol a run digit
            cases[f"n-{n}{tag}"] = [(k % 2) if k % 3 == 1 else 2 + (5 * k) % (nd - 1) for k in range(n)]
        cases["literals-only" + tag] = _literals(nd, 3000)
        cases["one-digit" + tag] = [1]

        # 256 chunks of 12 symbols; chunk 5 is digits only: its byte is the front of ITS start list, whatever position the
        # last literal of chunk 4 had
        symbols = _literals(nd, 256 * 12)
        symbols[59] = nd                      # the deepest position, just in front
        symbols[60:72] = [0] * 12
        assert cs.mtf_chunks(symbols, 256)[5:7] == [60, 72]
        cases["digits-only-chunk" + tag] = symbols

        # 256 chunks of 600 symbols (every chunk begins on a multiple of 8): digit sequences that begin at offsets 7, 8, 511,
        # 512 and 513 of a chunk -- across the eight symbols of a lane and the 512 of a tile -- and sequences of 5 from 509 on
        symbols = _literals(nd, 256 * 600)
        for chunk, offset in enumerate((7, 8, 511, 512, 513), start=1):
            symbols[600 * chunk + offset:600 * chunk + offset + 3] = [1, 0, 1]
        for chunk, offset in enumerate(range(506, 515), start=10):
            symbols[600 * chunk + offset:600 * chunk + offset + 5] = [0, 1, 1, 0, 1]
        starts = cs.mtf_chunks(symbols, 256)
        assert starts[:20] == [600 * t for t in range(20)]
        cases["digits-across-lanes-and-tiles" + tag] = symbols

        # runs just below, at and above the window (and twice the window, from where whole windows are skipped), each at every
        # output position mod 16, a literal behind
        symbols = []
        position = 0
        for c in (WINDOW - 1, WINDOW, WINDOW + 1, 2 * WINDOW - 1, 2 * WINDOW, 2 * WINDOW + 1, 3 * WINDOW + 17):
            for a in range(16):
                pad = (a - position) % 16 or 16
                symbols += _literals(nd, pad, len(symbols))
                symbols += cs.run_digits(c)
                position = (position + pad + c) % 16
        symbols += _literals(nd, 3)
        cases["runs-around-the-window" + tag] = symbols

        # two runs of 18 digits back to back: 262 143 bytes each, whole windows skipped
        cases["two-runs-of-18-digits" + tag] = [3] + [0] * 18 + [nd] + [0] * 18 + [2, 4]

        # literal and run of 1 in turn: no 16-byte unit gets its bytes from one lane
        cases["alternating" + tag] = [s for k in range(2500) for s in (2 + (3 * k) % (nd - 1), 0)]
    return cases


NEW = _new_cases()
Built = collections.namedtuple("Built", "symbols declared column out crc stream")


@functools.lru_cache(maxsize=None)
def built(name):
    nd = int(name.rsplit("@", 1)[1])
    declared = cs.D19 if nd == 19 else cs.D200
    c = cs._case(NEW[name], declared, cs.flat_tables(nd + 2))
    column = bz2parse.unmtf(c["symbols"], c["declared"])
    orig_ptr = (2 * len(column)) // 3
    _, out, crc = crafted.model_decode(column, orig_ptr)
    stream, _ = bz2enc.encode_block_from_symbols(c["symbols"], c["declared"], orig_ptr, crc, c["tables"], c["selectors"],
                                                 c["selectors_written"])
    return Built(c["symbols"], declared, column, out, crc, stream)


_ORACLE = {}


def oracle_record(oracle, name, stream):
    if name not in _ORACLE:
        _ORACLE[name] = oracle.decode_block(stream, 32)[0]
    return _ORACLE[name]


def check_column(name, dec, index, b, lanes):
    bad = first_difference(dec.debug_stage(index, 0), b.column)
    if bad is not None:
        from test_gpu_symbol_stages import symbol_of_column_byte
        k = symbol_of_column_byte(b.symbols[:-1], bad)
        raise AssertionError(f"{name}: column byte {bad} of {len(b.column)} differs: symbol {k} ({b.symbols[k]}), in the chunk of "
                             f"k_mtf lane {cs.mtf_lane_of(b.symbols[:-1], lanes, k)} of {lanes}")


@pytest.mark.parametrize("name", sorted(NEW))
def test_new_case(native, oracle, dec, switches, name):
    b = built(name)
    dec.set_input(b.stream)
    results, total = dec.decode_batch([32])
    check_column(name, dec, 0, b, cs.mtf_lanes(len(b.declared), 1, dec.variant == "mtf-256"))
    check_record(name, results[0], oracle_record(oracle, name, b.stream), b.crc, len(b.out))
    assert results[0]["data_offset"] == 0 and total == len(b.out)
    bad = first_difference(dec.copy_output(0, total), b.out)
    assert bad is None, f"{name}: payload differs from the model at byte {bad} of {len(b.out)}"


def test_new_cases_in_one_batch(native, oracle, dec, switches):
    """Every new case three times, shuffled: more than 64 entries, so k_mtf runs with 512 lanes per block (256 under mtf-256)
    and blocks of both instances sit side by side."""
    names = sorted(NEW)
    data = bytearray()
    entries = []
    for name in names:
        entries.append((name, len(data) * 8 + 32))
        data += built(name).stream
    entries = entries * 3
    order = np.random.default_rng(0xE7A).permutation(len(entries))
    entries = [entries[i] for i in order]
    assert 65 <= len(entries) <= 640
    want = {o: (name, built(name).out, built(name).crc) for name, o in entries}
    check_batch(oracle, dec, bytes(data), [o for _, o in entries], want)
    for k, (name, _) in enumerate(entries):
        lanes = cs.mtf_lanes(len(built(name).declared), len(entries), dec.variant == "mtf-256")
        check_column(name, dec, k, built(name), lanes)


# ---------------------------------------------------------------------------------------------------------------------
# (c) blocks that take the fallback whatever the switch says
# ---------------------------------------------------------------------------------------------------------------------
def _fallback_cases():
    cases = {}
    for nd in (19, 200):
        tag = f"@{nd}"
        cases["run-of-max-n-plus-1" + tag] = cs.run_digits(MAX_N + 1)
        # MAX_N bytes of runs and literals, then one literal more
        symbols = []
        for k in range(3000):
            symbols += [2 + k % (nd - 1)] + cs.run_digits(299)
        cases["max-n-and-a-literal" + tag] = symbols + [2]
        cases["21-digits" + tag] = [3] + [0] * 21 + [2]
        cases["33-digits" + tag] = [3] + [0] * 33 + [2, 4, 2]
    return cases


FALLBACK = _fallback_cases()


@functools.lru_cache(maxsize=None)
def fallback_stream(name):
    nd = int(name.rsplit("@", 1)[1])
    declared = cs.D19 if nd == 19 else cs.D200
    c = cs._case(FALLBACK[name], declared, cs.flat_tables(nd + 2))
    stream, _ = bz2enc.encode_block_from_symbols(c["symbols"], c["declared"], 0, 0x12345678, c["tables"], c["selectors"],
                                                 c["selectors_written"])
    return stream


@pytest.mark.parametrize("name", sorted(FALLBACK))
def test_fallback_block(native, oracle, dec, switches, name):
    stream = fallback_stream(name)
    want = oracle_record(oracle, "fallback " + name, stream)
    dec.set_input(stream)
    results, _ = dec.decode_batch([32])
    for key in RECORD_KEYS:
        assert results[0][key] == want[key], f"{name} ({dec.variant}): {key}: gpu {results[0][key]} != oracle {want[key]}"
