"""GPU suite: the decoder's back half -- table build, k_walk, k_link2, k_emit, k_replicate, k_rle, k_crc -- on the crafted
last columns of tests/crafted.py, against the plain model there and the oracle.  Every case is a valid stream that the
reference decodes (tests/golden/crafted_vectors.json), built to reach one branch: tests/test_crafted_streams.py asserts
on the CPU that it does.

Run on the GPU box: python -m pytest tests/test_gpu_decode_stages.py -m gpu -q --durations=0
"""
import numpy as np
import pytest

import crafted

pytestmark = pytest.mark.gpu

RECORD_KEYS = ("encoded_offset_bits", "encoded_size_bits", "decoded_size", "header_crc", "computed_crc", "bwt_length",
               "orig_ptr", "n_symbols", "is_eos", "is_eof", "status")

GPU_NAMES = crafted.NAMES
TABLE_NAMES = [name for name in crafted.small_names() if name.split("-")[0] in ("comb", "sorted", "random4", "random256",
                                                                                 "random2")]


@pytest.fixture(scope="module", params=["stages-kept", "as-shipped"])
def dec(native, request):
    """As in test_gpu_parity: once on a context that keeps the per-stage buffers addressable, once on one made the way the
    reader and the bench make theirs (R overlays L there, and k_replicate parks its period in the stash)."""
    keep = request.param == "stages-kept"
    d = native.Decoder(flags=native.Decoder.KEEP_STAGES if keep else 0)
    d.keeps_stages = keep
    yield d
    d.close()


def first_difference(got, want):
    if len(got) != len(want):
        return min(len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    bad = np.flatnonzero(a != b)
    return int(bad[0]) if bad.size else None


def pre_index_of_output(pre, k):
    """The pre-RLE1 byte that output byte k comes from (the count byte for the bytes a count expands to)."""
    produced, run, prev = 0, 0, -1
    for i, b in enumerate(pre):
        if run == 4:
            produced += b
            run, prev = 0, -1
        else:
            produced += 1
            run = run + 1 if b == prev else 1
            prev = b
        if produced > k:
            return i
    return len(pre) - 1


def check_record(name, r, od, crc, size):
    for key in RECORD_KEYS:
        assert r[key] == od[key], f"{name}: {key}: gpu {r[key]} != oracle {od[key]}"
    assert (r["status"], r["computed_crc"], r["header_crc"], r["decoded_size"]) == (0, crc, crc, size), (name, r)


def check_stages(name, dec, index):
    """The three stage buffers of block `index` of the last batch against the column and the model."""
    last, orig_ptr = crafted.column(name)
    pre = crafted.model(name)[0]
    g = crafted.geometry(name)
    n = len(last)
    bad = first_difference(dec.debug_stage(index, 0), last)
    assert bad is None, f"{name}: L column differs at {bad}"
    # the packed table of k_bwt_build / k_bwt_rank: LF << 8 | byte | MARK, with LF_MASK = 0xFFFFF and MARK = 0x80000000
    # of bz2_kernels.hip.h; marked are the segment starts, every stride-th index and origPtr
    table = np.frombuffer(dec.debug_stage(index, 1), dtype="<u4")
    lf = crafted.inverse_tables(last)[1]
    column = np.frombuffer(last, dtype=np.uint8)
    marks = np.zeros(n, dtype=bool)
    marks[::g["stride"]] = True
    marks[orig_ptr] = True
    for what, got, want in (("byte", table & 0xFF, column), ("LF", (table >> 8) & 0xFFFFF, lf),
                            ("MARK", (table & 0x80000000) != 0, marks), ("unused bits", table & 0x70000000, 0)):
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (f"{name}: table {what} differs at index {int(wrong[0])}: gpu {got[wrong[0]]}"
                                 f" (entry {int(table[wrong[0]]):#x}), {wrong.size} entries in all")
    bad = first_difference(dec.debug_stage(index, 2), pre)
    assert bad is None, f"{name}: inverse BWT differs from the model at {crafted.describe(g, bad)}"


def check_case(name, native, oracle, dec, stages):
    enc = crafted.stream(name)
    pre, out, crc = crafted.model(name)
    od = oracle.decode_block(enc, 32)[0]
    assert native.find_magic(enc) == [32]
    dec.set_input(enc)
    results, total = dec.decode_batch([32])
    check_record(name, results[0], od, crc, len(out))
    if stages:
        check_stages(name, dec, 0)
    assert results[0]["data_offset"] == 0 and total == len(out)
    bad = first_difference(dec.copy_output(0, total), out)
    if bad is not None:
        where = crafted.describe(crafted.geometry(name), pre_index_of_output(pre, bad))
        raise AssertionError(f"{name}: payload differs from the model at byte {bad} of {len(out)}; {where}")


@pytest.mark.parametrize("name", GPU_NAMES)
def test_crafted_block(native, oracle, dec, name):
    check_case(name, native, oracle, dec, dec.keeps_stages)


@pytest.mark.parametrize("split", ["by-batch-size", "1", "2", "4"])
def test_table_build_variants(native, oracle, split, monkeypatch):
    """k_bwt_build (one workgroup per block) and k_bwt_count + k_bwt_rank with 2 and 4 slices per block, and what a batch
    of one block takes by itself (8 slices), as test_huffman_stage_variants selects them: the combs (one symbol holds
    N - 16 entries: the worst case for the per-slice histograms and ranks), the sorted column and the random ones."""
    if split != "by-batch-size":
        monkeypatch.setenv("MI355X_BZ2_BWT_SPLIT", split)
    d = native.Decoder(flags=native.Decoder.KEEP_STAGES)
    try:
        for name in TABLE_NAMES:
            check_case(name, native, oracle, d, True)
    finally:
        d.close()


def check_batch(oracle, d, data, offsets, want):
    """One batch: results in the caller's order, data_offset running, records against the oracle, payloads and CRCs
    against `want` (offset -> (name, bytes, crc))."""
    d.set_input(data)
    results, total = d.decode_batch(offsets)
    out = d.copy_output(0, total)
    records = {}
    pos = 0
    for k, (o, r) in enumerate(zip(offsets, results)):
        name, payload, crc = want[o]
        if o not in records:
            records[o] = oracle.decode_block(data, o)[0]
        check_record(f"entry {k} ({name})", r, records[o], crc, len(payload))
        assert r["data_offset"] == pos, (k, name)
        bad = first_difference(out[pos:pos + len(payload)], payload)
        assert bad is None, f"entry {k} ({name}) at output offset {pos} (mod 64: {pos % 64}): payload differs at byte {bad}"
        pos += len(payload)
    assert pos == total


def test_tiny_blocks_at_every_output_alignment(native, oracle, dec):
    """130 blocks of 1 ... 130 decoded bytes in one batch: out_off takes every residue mod 64 (k_rle's writes, k_crc's
    reads of the expansion)."""
    data, parts = crafted.tiny_blocks_file()
    offsets = oracle.find_magic(data)
    assert native.find_magic(data) == offsets and len(offsets) == len(parts)
    want = {o: (f"{len(p)} bytes", p, crafted.crc32_bzip2(p)) for o, p in zip(offsets, parts)}
    check_batch(oracle, dec, data, offsets, want)


def crafted_batch_inputs():
    data, entries = crafted.crafted_batch()
    want = {o: (name,) + crafted.model(name)[1:] for name, o in entries}
    return data, [o for _, o in entries], want


def test_crafted_batch(native, oracle, dec):
    """Every crafted block with N <= 70 000, each twice, shuffled: a k_walk claim of 256 segments spans many blocks of 1-3
    segments beside blocks with thousands; blocks with and without k_replicate's work in one launch."""
    data, offsets, want = crafted_batch_inputs()
    check_batch(oracle, dec, data, offsets, want)
    if dec.keeps_stages:
        names = {o: name for name, o in crafted.crafted_batch()[1]}
        for k in range(0, len(offsets), 7):
            check_stages(names[offsets[k]], dec, k)


def test_crafted_batch_beside_other_contexts(native, oracle):
    """The same batch on a context as shipped with three others alive, as test_batches_beside_other_contexts: the planner
    takes its crowd settings."""
    data, offsets, want = crafted_batch_inputs()
    others = [native.Decoder() for _ in range(3)]
    d = native.Decoder()
    try:
        check_batch(oracle, d, data, offsets, want)
    finally:
        d.close()
        for other in others:
            other.close()
