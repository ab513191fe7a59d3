"""GPU suite: the decoder's front half -- scan_parse, k_hscan<1>, k_hscan_spec<4/8>, k_hsym, k_mtf in both strides with 256,
512 and 1 024 lanes -- on the crafted symbol streams of tests/crafted_symbols.py, against the plain model there and the
oracle.  Every case is a valid stream that the reference decodes (tests/golden/crafted_symbols_vectors.json), built to reach
one branch: tests/test_crafted_symbols.py asserts on the CPU that it does.  On a context that keeps its stages the scan's
hand-off is checked by itself: group starts (stage 3), ScanMeta (4), selectors (5), and the column behind k_mtf (0).

Run on the GPU box: python -m pytest tests/test_gpu_symbol_stages.py -m gpu -q --durations=0
"""
import struct

import numpy as np
import pytest

import crafted_symbols as cs
from test_gpu_decode_stages import check_batch, check_record, first_difference

pytestmark = pytest.mark.gpu

# what a context is made under: the scan by batch size (eight waves for a batch of one), k_hscan<1>, k_hscan_spec<4>, <8>;
# k_mtf with 256 lanes; and a context as shipped (no stage buffers: records and payload only)
VARIANTS = {
    "scan-by-batch-size": {},
    "scan-1": {"MI355X_BZ2_SCAN_WAVES": "1"},
    "scan-4": {"MI355X_BZ2_SCAN_WAVES": "4"},
    "scan-8": {"MI355X_BZ2_SCAN_WAVES": "8"},
    "mtf-256": {"MI355X_BZ2_MTF_NARROW": "1"},
    "as-shipped": {},
}
SWITCHES = ("MI355X_BZ2_SCAN_WAVES", "MI355X_BZ2_MTF_NARROW")
BIG = set(cs.big_names())


def _context(native, variant):
    """The switches are set, then the context is made (they are read per batch: every test sets them again)."""
    with pytest.MonkeyPatch.context() as mp:
        for key in SWITCHES:
            mp.delenv(key, raising=False)
        for key, value in VARIANTS[variant].items():
            mp.setenv(key, value)
        keep = variant != "as-shipped"
        d = native.Decoder(flags=native.Decoder.KEEP_STAGES if keep else 0)
        d.keeps_stages = keep
        d.variant = variant
        yield d
        d.close()


@pytest.fixture(scope="module", params=list(VARIANTS))
def dec(native, request):
    yield from _context(native, request.param)


@pytest.fixture(scope="module", params=[v for v in VARIANTS if v != "as-shipped"])
def dec_for_big(native, request):
    """The full block and the long runs go once through each scan variant and through the narrow k_mtf."""
    yield from _context(native, request.param)


def _set(monkeypatch, variant):
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, value in VARIANTS[variant].items():
        monkeypatch.setenv(key, value)


@pytest.fixture
def switches(dec, monkeypatch):
    _set(monkeypatch, dec.variant)


_ORACLE_RECORDS = {}


def oracle_record(oracle, name):
    if name not in _ORACLE_RECORDS:
        _ORACLE_RECORDS[name] = oracle.decode_block(cs.model(name).stream, 32)[0]
    return _ORACLE_RECORDS[name]


def symbol_of_column_byte(symbols, index):
    """The symbol that wrote byte `index` of the column (the last digit of a run for the bytes of the run)."""
    produced, run, weight = 0, 0, 1
    for k, s in enumerate(symbols):
        if s <= 1:
            run += weight << s
            weight <<= 1
            if k + 1 < len(symbols) and symbols[k + 1] <= 1:
                continue
            produced += run
            run, weight = 0, 1
        else:
            produced += 1
        if produced > index:
            return k
    return len(symbols) - 1


def check_scan_stages(name, dec, index, stream_bit, input_bits, lanes):
    """Block `index` of the last batch, whose stream starts at bit `stream_bit` of an input of `input_bits` bits: what the scan
    hands to k_hsym and what k_mtf leaves, against the model."""
    m, c = cs.model(name), cs.case(name)
    n_groups = len(m.group_starts)
    pos_base, size_bits, found_groups, terminal, symbol_count = struct.unpack("<QIIII", dec.debug_stage(index, 4)[:24])
    assert (found_groups, terminal, symbol_count) == (n_groups, 1, len(m.declared)), \
        f"{name}: ScanMeta n_groups {found_groups} terminal {terminal} symbol_count {symbol_count}, model {n_groups} 1 {len(m.declared)}"
    assert pos_base == (stream_bit + m.group_starts[0]) & ~31 and pos_base + size_bits == input_bits, (name, pos_base, size_bits)
    found = pos_base + np.frombuffer(dec.debug_stage(index, 3), dtype="<u4")[:n_groups].astype(np.int64)
    want = stream_bit + np.asarray(m.group_starts, dtype=np.int64)
    bad = np.flatnonzero(found != want)
    assert bad.size == 0, (f"{name}: group {int(bad[0])} of {n_groups} (table {c['selectors'][bad[0]]}) starts at bit "
                           f"{int(want[bad[0]])}, the scan found {int(found[bad[0]])}; {bad.size} groups differ")
    n_sel = len(m.selectors_written)
    bad = first_difference(dec.debug_stage(index, 5)[:n_sel], bytes(m.selectors_written))
    assert bad is None, f"{name}: selector {bad} of {n_sel} is {m.selectors_written[bad]}, the scan wrote otherwise"
    bad = first_difference(dec.debug_stage(index, 0), m.column)
    if bad is not None:
        k = symbol_of_column_byte(m.symbols[:-1], bad)
        raise AssertionError(f"{name}: column byte {bad} of {len(m.column)} differs: symbol {k} ({m.symbols[k]}) of group {k // 50}, "
                             f"in the chunk of k_mtf lane {cs.mtf_lane_of(m.symbols[:-1], lanes, k)} of {lanes}")


def check_case(name, native, oracle, dec):
    m = cs.model(name)
    assert native.find_magic(m.stream) == [32]
    dec.set_input(m.stream)
    results, total = dec.decode_batch([32])
    check_record(name, results[0], oracle_record(oracle, name), m.crc, len(m.out))
    if dec.keeps_stages:
        lanes = cs.mtf_lanes(len(m.declared), 1, dec.variant == "mtf-256")
        check_scan_stages(name, dec, 0, 0, len(m.stream) * 8, lanes)
    assert results[0]["data_offset"] == 0 and total == len(m.out)
    bad = first_difference(dec.copy_output(0, total), m.out)
    assert bad is None, f"{name}: payload differs from the model at byte {bad} of {len(m.out)}"


@pytest.mark.parametrize("name", [name for name in cs.NAMES if name not in BIG])
def test_symbol_case(native, oracle, dec, switches, name):
    check_case(name, native, oracle, dec)


@pytest.mark.parametrize("name", sorted(BIG))
def test_big_symbol_case(native, oracle, dec_for_big, monkeypatch, name):
    _set(monkeypatch, dec_for_big.variant)
    check_case(name, native, oracle, dec_for_big)


def test_symbol_batch(native, oracle, dec, switches):
    """Every case whose column has at most 70 000 bytes, each twice, shuffled: more than 64 entries, so k_mtf runs with 512
    lanes per block (256 under mtf-256), blocks of 2 and of 1 025 groups side by side in the scan and in k_hsym."""
    data, entries = cs.symbol_batch()
    want = {o: (name, cs.model(name).out, cs.model(name).crc) for name, o in entries}
    check_batch(oracle, dec, data, [o for _, o in entries], want)
    if dec.keeps_stages:
        for k in range(0, len(entries), 3):
            name, o = entries[k]
            lanes = cs.mtf_lanes(len(cs.model(name).declared), len(entries), dec.variant == "mtf-256")
            check_scan_stages(name, dec, k, o - 32, len(data) * 8, lanes)
