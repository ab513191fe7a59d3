"""CPU suite: the crafted last columns of tests/crafted.py.  For every case the plain model (crafted.model_decode), the
oracle, CPython's bz2 and the recorded answer of the real reference (tests/golden/crafted_vectors.json, written by
tests/golden/make_golden_crafted.py from oracle/_ref/ref_bz2 probe) agree, and the case has the walk geometry it is
there for.  The GPU side of the same cases is tests/test_gpu_decode_stages.py."""
import bz2
import hashlib
import json
import os
import random

import pytest

from conftest import ROOT
import bz2enc
import crafted
import datagen
from test_oracle import fnv64

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "crafted_vectors.json")
GOLDEN = json.load(open(GOLDEN_PATH))

# bz2enc.encode_block became a caller of encode_block_from_bwt: the streams it wrote before must not change by a byte
STREAM_HASHES = {
    "exotic alphabet62-deep-tail": "66b5ec30fdab0df4cb30ee9ec645e164a55b76bc77affd9350fc6896e2436945",
    "exotic declared-unused-extra-selectors": "6d19a638d74889eb3db9db1d442de3fa20b7ef49f71b6e0211a7a417177b0c4b",
    "exotic rotating-codes-5tables": "00c9ec9ef6a190a03f07b7a5c974ba23550eb02cf803a87a81bab373fca94c1a",
    "exotic skew20-2tables": "e295ebb4284b8f3f4af6bed496c68470c040662fe50f8130228b0456a2f55f80",
    "exotic skew20-frequent-long-6tables": "a75c0735899ae9b7f156e9700a6348172247745a4909dcd78ffc9cfb2264906f",
    "exotic tiny": "c770d0d7fcc353d0922c457326667f63bca9cb427cc1f5005b6789d57b15b5f1",
    "faulty data-overflow": "731ac8f583b6854e23abcf5bb147717b4992883b7335480fb67accaeeb241e9d",
    "faulty group-count-1": "7293e57bfd658b14d234d0aff322217c8c40b6095597c1105bb81e5ea5c74445",
    "faulty group-count-7": "465a405f88d357fa714c4266dffe18417a3e90159bd0bf445cc3802504fbe1c3",
    "faulty origptr-900001": "11e7804a16c0e32b2c72e08f6e573deb417392502a531610a22f01eead557e36",
    "faulty origptr-equals-n": "42ab1e82eb83e99b7157a18fcebe61cf1a986f10bce0110438bd324b03fb5528",
    "faulty randomized-bit": "46c0e29a0569c134fda5cbfd451ad28b363b58a4e12c4ab4b714f4263ba78e64",
    "faulty run-overflow": "2ab4488bfe432468de12f71aec9aec90ab87f7665f23a1e806fd66f2462b5315",
    "faulty selector-count-0": "5861e2454615ff436bbe9f5e0f9cfca3c9aac58ba162ba8b6db7fab520f83a93",
    "faulty selectors-run-out": "b9c1eab4455dee67ee3810df03f51ce9f48ec936d9fa54e5d1ded64378c77dfe",
}

# Blocks that end in four equal bytes with no count behind them: libbz2 refuses them, the reference decodes them (the
# first to 16 469 bytes) and is our specification.  rot-15 is one by arithmetic: b, then 14 = 5 + 5 + 4 times a.
REFUSED_BY_LIBBZ2 = {"rle-ends-in-four-equal", "rot-15"}


def test_encode_block_streams_are_unchanged():
    got = {f"exotic {name}": hashlib.sha256(enc).hexdigest() for name, (raw, enc) in datagen.exotic_streams().items()}
    got.update({f"faulty {name}": hashlib.sha256(enc).hexdigest() for name, (enc, st) in datagen.faulty_streams().items()})
    assert got == STREAM_HASHES


def test_bwt_numpy_equals_the_sorting_bwt():
    r = random.Random(0xB37)
    for case in range(150):
        n = r.randint(1, 2000)
        s = bytes(r.randrange(r.choice([1, 2, 3, 4, 256])) for _ in range(n))
        if case % 5 == 0:
            s = (s[:r.randint(1, 7)] * n)[:n]         # periodic: identical rotations, ties
        assert bz2enc.bwt_numpy(s) == bz2enc.bwt(s), (case, n)


def test_model_pieces():
    assert crafted.crc32_bzip2(b"123456789") == 0xFC891918 and crafted.crc32_bzip2(b"") == 0
    data = datagen.runs(3000, 5, 40)
    assert crafted.crc32_bzip2(data) == bz2enc.crc32_bzip2(data) ^ 0xFFFFFFFF
    # the model inverts the sorting BWT + RLE1 of bz2enc, runs of every length from 1 to 4 + 255 and beyond included
    for raw in (data, b"x" * 1000, b"ab" * 300, bytes(range(256)), b"aaaa", b"aaaab", b"\x05" * 9 + b"\x04" * 4):
        pre = bz2enc.rle1(raw)
        last, orig_ptr = bz2enc.bwt(pre)
        assert crafted.model_decode(last, orig_ptr) == (pre, raw, bz2enc.crc32_bzip2(raw) ^ 0xFFFFFFFF)


def test_model_decodes_a_libbz2_block(oracle):
    raw = datagen.text_like(60_000, 5) + datagen.runs(20_000, 6)
    enc = datagen.compress(raw, 1)
    d, payload, lcol, rle = oracle.decode_block(enc, 32, want_stages=True)
    assert crafted.model_decode(lcol, d["orig_ptr"]) == (rle, raw, d["header_crc"])
    g = crafted.walk_geometry(lcol, d["orig_ptr"])
    assert g["c"] == g["n"] == len(lcol) and g["nchain"] == g["nseg"]


@pytest.mark.parametrize("name", crafted.NAMES)
def test_model_oracle_and_libbz2_agree(oracle, name):
    last, orig_ptr = crafted.column(name)
    pre, out, crc = crafted.model(name)
    enc = crafted.stream(name)
    if name in crafted.RLE_NAMES:
        assert pre == crafted.rle_streams()[name]           # the column really is the BWT of the crafted stream
    d, payload, lcol, rle = oracle.decode_block(enc, 32, want_stages=True)
    assert (d["status"], d["bwt_length"], d["orig_ptr"], d["header_crc"], d["computed_crc"], d["decoded_size"]) == \
           (0, len(last), orig_ptr, crc, crc, len(out)), d
    assert 0 <= len(enc) * 8 - 32 - d["encoded_size_bits"] - 80 < 8      # stream header, block, end-of-stream + CRC, padding
    assert lcol == last and rle == pre and payload == out
    st, whole, block_map, garbage = oracle.decode_file(enc)
    assert st == 0 and whole == out and not garbage
    assert (name in REFUSED_BY_LIBBZ2) == (_edge_counts(name)[1] == 4)
    if name in REFUSED_BY_LIBBZ2:
        with pytest.raises((OSError, ValueError)):
            bz2.decompress(enc)
    else:
        assert bz2.decompress(enc) == out


def _edge_counts(name):
    """Indices of the count bytes of an RLE case, by the model's own state machine."""
    pre = crafted.model(name)[0]
    counts, run, prev = [], 0, -1
    for i, b in enumerate(pre):
        if run == 4:
            counts.append(i)
            run, prev = 0, -1
            continue
        run = run + 1 if b == prev else 1
        prev = b
    return counts, run


@pytest.mark.parametrize("name", crafted.NAMES)
def test_geometry_reaches_its_branch(name):
    """Conditions, not measurements: what each case must show for the branch it is there for (bz2_walk.hip.h,
    bz2_kernels.hip.h).  If one fails after a constant changed there, the case list is stale."""
    g = crafted.geometry(name)
    n = g["n"]
    assert g["stride"] == max(16, -(-n // crafted.KMAX)) and g["nseg"] <= crafted.KMAX + 1
    if name == "comb-40000-5":
        # k_emit: put()'s oversized piece, the re-walk of a segment beyond its stash; a block of nearly all length-1 segments
        assert (g["c"], g["nseg"], g["first"], g["ones"], g["longest"]) == (n, 2501, g["k0"], 2499, 25001)
        assert g["worst_piece"] == 25256 > crafted.EMIT_STAGE and g["first_extra"]
    elif name == "comb-40000-0":
        assert (g["nseg"], g["k0"], g["first"], g["longest"], g["c"]) == (2500, 2500, 0, 37501, n)
        assert g["worst_piece"] > crafted.EMIT_STAGE
    elif name == "comb-65537-5":
        assert (g["c"], g["n_mod_c"], g["nchain"]) == (32768, 1, 1)          # one segment is the whole cycle
    elif name == "comb-65537-0":
        assert (g["c"], g["n_mod_c"], g["ones"], g["longest"]) == (32769, 32768, 4096, 28673)
    elif name == "comb-4096-2048":
        assert g["first"] == 128 == crafted.LINK_SPLIT and not g["first_extra"] and g["nseg"] == 256
    elif name == "comb-2048-7":
        assert g["nseg"] == 129 and g["first"] == g["k0"] == 128 and not g["first_extra"]
    elif name == "comb-544000-5":
        assert (g["stride"], g["nseg"], g["longest"], g["c"]) == (17, 32001, 352001, n)
    elif name.startswith("rot-") and name.count("-") == 1:
        want_k0 = {1: 1, 2: 1, 15: 1, 16: 1, 17: 2, 31: 2, 32: 2, 33: 3, 2047: 128, 2048: 128, 2049: 129}
        assert g["k0"] == want_k0[n] and g["longest"] <= g["stride"] and g["c"] == n
    elif name == "rot-524288-0":
        assert (g["nseg"], g["first"], g["stride"]) == (32768, 0, 16)
    elif name == "rot-524288-5":
        assert (g["nseg"], g["first"], g["stride"]) == (crafted.KMAX + 1, 32768, 16)       # the maximum
    elif name == "rot-524289-5":
        assert (g["stride"], g["nseg"]) == (17, 30842)
    elif name == "rot-900000-5":
        assert (g["stride"], g["nseg"]) == (28, 32144)
    elif name == "sorted-30000":
        assert g["c"] == 1 and g["nchain"] == 1                                            # LF is the identity
    elif name.startswith("random"):
        # several cycles and N no multiple of the one through origPtr: k_replicate's shifted layout, with status 0
        assert 1 < g["c"] < n and g["n_mod_c"] != 0 and 1 < g["nchain"] < g["nseg"]
        if name == "random256-50000":
            assert g["first"] == 4096 // 16 and not g["first_extra"]                       # aligned origPtr
        if name == "random4-524288":
            assert g["nseg"] == crafted.KMAX + 1 and g["over_stash"] >= 1
    else:
        assert name in crafted.RLE_NAMES
        counts, final_run = _edge_counts(name)
        if name.startswith("rle-count") and "-at-" in name:
            want = int(name.rsplit("-", 1)[1])
            assert counts == [want] and crafted.model(name)[0][want] == int(name.split("-")[1][5:])
        elif name == "rle-run-at-every-edge":
            assert counts == [crafted.RLE_CHUNK, crafted.RLE_WAVE, crafted.RLE_TILE, 2 * crafted.RLE_TILE] and n == 33_000
        elif name == "rle-ends-in-four-equal":
            assert n == 16_404 and final_run == 4 and counts == [crafted.RLE_TILE - 1] and len(crafted.model(name)[1]) == 16_469
        elif name.startswith("rle-ends-in-three-equal"):
            assert n == int(name.rsplit("-", 1)[1]) and final_run == 3 and counts == []
        elif name == "rle-count-equals-value":
            pre = crafted.model(name)[0]
            assert len(counts) == 2 and pre[counts[0]] == pre[counts[0] - 1] == pre[counts[0] + 1] == 0x30
        elif name == "rle-back-to-back":
            assert len(counts) == 3401 and counts[:2] == [4, 9]
        else:
            raise AssertionError(f"no condition written for {name}")


def test_case_list_covers_the_edges():
    names = set(crafted.NAMES)
    for p in crafted.RLE_EDGE_POSITIONS:
        assert any(name.startswith("rle-count") and name.endswith(f"-at-{p}") for name in names), p
    # every position of a run (four bytes and the count) across a chunk, wave and tile edge of k_rle
    assert crafted.RLE_EDGE_POSITIONS == [e + d for e in (crafted.RLE_CHUNK, crafted.RLE_WAVE, crafted.RLE_TILE)
                                          for d in range(-1, 5)]
    assert len(crafted.small_names()) == len(GOLDEN["cases"]) and "rle-ends-in-four-equal" in GOLDEN["cases"]


def test_batches(oracle):
    """The two batches of the GPU test, on the CPU: the tiny blocks' decoded sizes are 1 ... 130 (their output offsets
    then take every residue mod 64), the crafted batch names >= 64 blocks and every offset is a block of its case."""
    data, parts = crafted.tiny_blocks_file()
    offs = oracle.find_magic(data)
    assert [len(p) for p in parts] == list(range(1, 131)) and len(offs) == 130
    assert bz2.decompress(data) == b"".join(parts)
    starts = [sum(range(1, k)) for k in range(1, 131)]
    assert {s % 64 for s in starts} == set(range(64))
    data, entries = crafted.crafted_batch()
    assert len(entries) >= 64 and sorted({o for _, o in entries}) == oracle.find_magic(data)
    for name, off in entries[:len(entries) // 2]:
        d, payload = oracle.decode_block(data, off)
        assert d["status"] == 0 and payload == crafted.model(name)[1], name


@pytest.mark.parametrize("name", sorted(GOLDEN["cases"]))
def test_reference_answers(oracle, name, tmp_path):
    """What the real reference said about the very same stream (recorded), against the oracle and the model; and against the
    reference itself where its binary is present."""
    gold = GOLDEN["cases"][name]
    enc = crafted.stream(name)
    assert hashlib.sha256(enc).hexdigest() == gold["enc_sha256"], "builder drifted: rerun tests/golden/make_golden_crafted.py"
    assert gold["verdict"] == "OK"
    pre, out, crc = crafted.model(name)
    d, payload = oracle.decode_block(enc, 32)
    assert (d["status"], d["encoded_size_bits"], d["header_crc"], d["computed_crc"], d["decoded_size"], fnv64(payload)) == \
           (0, gold["size"], gold["header_crc"], gold["calc_crc"], gold["decoded"], gold["fnv64"])
    assert (crc, len(out), fnv64(out)) == (gold["calc_crc"], gold["decoded"], gold["fnv64"])
    if oracle.ref_available():
        p = tmp_path / "case.bz2"
        p.write_bytes(enc)
        assert crafted.parse_probe(oracle.ref_run("probe", p, 32)) == {k: v for k, v in gold.items() if k != "enc_sha256"}
