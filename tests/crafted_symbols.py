"""Crafted symbol streams for the decoder's front half: scan_parse, k_hscan<1>, k_hscan_spec<4/8>, k_hsym (bz2_hscan.hip.h)
and k_mtf in both strides and its three lane counts (bz2_stage1.hip.h).

libbz2's output is benign for everything that code guesses: group lengths drift slowly, eight groups never reach
SPEC_REACH, long codes are rare in mid-block.  The format lets a block carry ANY symbols under ANY 2..6 complete tables of
1..20-bit codes with any selectors (bz2enc.encode_block_from_symbols), and the reference decodes them all.  This module holds
  - the cases: symbols, declared byte values, tables and selectors, each built to reach one branch,
  - the model: the column is bz2parse.unmtf of the symbols, everything behind it crafted.model_decode, the selectors and
    group starts are the encoder's,
  - hscan_plan / spec_plan / selector_plan / mtf_plan: the planning rules of k_hscan<1>, k_hscan_spec<K>, scan_parse's
    selector pass and k_mtf's chunk rule and byte sink restated as integer rules, so that every case can assert ON THE CPU
    that it reaches the branch it is there for (a changed constant fails the CPU test instead of silently leaving a
    branch unreached).
Plain Python + numpy: no product, no oracle."""
import collections
import functools
import itertools
import random

import numpy as np

import bz2enc
import bz2parse
import crafted

# the constants of bz2_hscan.hip.h / bz2_stage1.hip.h / bz2_plan.hpp that the rules below restate
SCAN_MAX_SPAN = 1024
SCAN_ROWS = SCAN_MAX_SPAN // 64
SCAN_LUT_BITS = 10
SCAN_RING_ENTRIES = 256
SPEC_REACH = 32 * SCAN_RING_ENTRIES - 4700        # K = 4 and 8 share the 256-entry ring
GROUP_SYMS = 50
MAX_SCAN_GROUPS = 18002
SYM_GROUPS_PER_WORKGROUP = 256 * 4               # k_hsym: threads x SYM_CHUNKS
MTF_SMALL_ENTRIES = 128                          # declared values up to which a block takes k_mtf<144>
MAX_N = 900_000
OUT, TERM = "out", "term"

assert SPEC_REACH == 3492


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def skew(ranking):
    """Lengths 1, 2, ... 19, 20, 20 along `ranking` (a permutation of an alphabet of 21)."""
    assert sorted(ranking) == list(range(21))
    lengths = [0] * 21
    for i, s in enumerate(ranking):
        lengths[s] = min(i + 1, 20)
    return lengths


# literal 2 has 1 bit ... literal 18 has 17, the run digits 18 and 19, literal 19 and the end of block 20 (0xFFFFE, 0xFFFFF)
T_UP = skew(list(range(2, 19)) + [0, 1, 19, 20])
# the literals the other way round: literal 18 has 1 bit ... literal 2 has 17
T_DOWN = skew(list(range(18, 1, -1)) + [1, 0, 19, 20])
# the end of block has the one-bit code, literal 19 is 1^20
T_ONES = skew([20] + list(range(0, 20)))


def shuffled_tables(seed, count=6):
    """`count` tables 1..19, 20, 20 over shuffled rankings."""
    r = random.Random(seed)
    tables = []
    for _ in range(count):
        ranking = list(range(21))
        r.shuffle(ranking)
        tables.append(skew(ranking))
    return tables


def flat_tables(alphabet):
    """Two complete codes of near-equal lengths, the short codes on the low and on the high symbols."""
    up = crafted.flat_lengths(0, alphabet, list(range(alphabet, 0, -1)))
    down = crafted.flat_lengths(1, alphabet, list(range(alphabet)))
    return [up, down]


def group_of_bits(bits, table=T_UP):
    """50 literals (symbols >= 2) whose codes under `table` take `bits` bits in all."""
    by_length = {}
    for s in range(2, 20):
        by_length.setdefault(table[s], s)
    lengths = [1] * GROUP_SYMS
    left = bits - GROUP_SYMS
    assert 0 <= left <= 19 * GROUP_SYMS
    k = 0
    while left >= 19:
        lengths[k] = 20
        left -= 19
        k += 1
    if left in (17, 18):                # no literal of 18 or 19 bits
        lengths[k] = 17
        left -= 16
        k += 1
    if left:
        lengths[k] = 1 + left
    assert sum(lengths) == bits
    return [by_length[l] for l in lengths]


# ---------------------------------------------------------------------------------------------------------------------
# cases: name -> dict(symbols without the end of block, declared, tables, selectors_written or None)
# ---------------------------------------------------------------------------------------------------------------------
D19 = list(range(1, 20))
D200 = list(range(1, 201))


def _case(symbols, declared, tables, selector_fn=None, selectors=None, surplus=()):
    symbols = list(symbols) + [len(declared) + 1]
    n_sel = -(-len(symbols) // GROUP_SYMS)
    if selectors is None:
        selectors = [(selector_fn(g) if selector_fn else g % len(tables)) for g in range(n_sel)]
    assert len(selectors) == n_sel and 2 <= len(tables) <= 6
    return {"symbols": symbols, "declared": list(declared), "tables": tables, "selectors": list(selectors),
            "selectors_written": list(selectors) + list(surplus)}


def _scan_cases():
    cases = {}
    # 70 groups of 50 codes of 20 bits: 0xFFFFE, the deepest literal
    cases["long-1000"] = _case([19] * (70 * 50), D19, [T_UP, T_DOWN], lambda g: 0)
    # 800-bit groups: the longest that still leave room for eight windows in a span, so SPEC_REACH cuts the unit
    cases["long-800"] = _case(group_of_bits(800) * 40, D19, [T_UP, T_DOWN], lambda g: 0)
    cases["all-ones"] = _case([19] * (70 * 50), D19, [T_ONES, T_DOWN], lambda g: 0)
    cases["short-50"] = _case([2] * (200 * 50), D19, [T_UP, T_DOWN], lambda g: 0)
    for k in range(15):
        cases[f"jump-{k}"] = _case([2] * (50 * k) + [19] * 50, D19, [T_UP, T_DOWN], lambda g: 0)
    # two tables in turn; per table 50, 75, ... 1 000 and down again
    steps = list(range(50, 1001, 25)) + list(range(975, 49, -25)) + [50] * 6
    symbols = []
    for bits in steps:
        symbols += group_of_bits(bits, T_UP) + group_of_bits(bits, T_DOWN)
    cases["staircase"] = _case(symbols, D19, [T_UP, T_DOWN], lambda g: g % 2)
    # six tables
    r = random.Random(66)
    selectors = [(5 * g + 1) % 6 for g in range(150)]
    selectors[56:72] = [3] * 16          # across 63/64
    selectors[120:136] = [2] * 16        # across 127/128
    selectors[136:150] = [4] * 14
    cases["six-tables"] = _case([r.randrange(2, 20) for _ in range(149 * 50 + 17)], D19, shuffled_tables(6), None, selectors)
    for groups in (63, 64, 65, 128):
        r = random.Random(groups)
        cases[f"groups-{groups}"] = _case([r.choice((2, 2, 2, 3, 4, 5, 9)) for _ in range((groups - 1) * 50 + 10)], D19,
                                          [T_UP, T_DOWN], lambda g: (g // 3) % 2)
    for n in (3200, 3199):
        r = random.Random(n)
        name = "eob-alone-3200" if n == 3200 else "eob-last-3199"
        cases[name] = _case([r.choice((2, 3, 4, 6, 18)) for _ in range(n)], D19, [T_UP, T_DOWN], lambda g: (g // 2) % 2)
    # literals of exactly 9, 10, 11 and 12 bits, the two tables a bit apart
    r = random.Random(1011)
    lut_a = skew([2, 3, 4, 5, 6, 7, 8, 0, 9, 10, 11, 12, 1, 13, 14, 15, 16, 17, 18, 19, 20])     # 9..12: symbols 9, 10, 11, 12
    lut_b = skew([18, 17, 16, 15, 14, 13, 8, 7, 1, 9, 10, 11, 12, 0, 6, 5, 4, 3, 2, 19, 20])     # 10..13: symbols 9, 10, 11, 12
    cases["lut-edge"] = _case([r.choice((9, 10, 10, 11, 11, 12)) for _ in range(40 * 50 + 31)], D19, [lut_a, lut_b])
    # surplus selectors: their move-to-front positions are written as they are, codes of 1 to 6 bits
    r = random.Random(2048)
    real = [(5 * g + 1) % 6 for g in range(71)]
    order = list(range(6))
    for s in real:
        order.remove(s)
        order.insert(0, s)
    surplus = []
    for k in range(2600):
        p = (0, 5, 1, 4, 2, 3, 0, 0, 5, 5)[k % 10] if k % 7 else r.randrange(6)
        surplus.append(order.pop(p))
        order.insert(0, surplus[-1])
    r = random.Random(70)
    cases["selectors-rounds"] = _case([r.randrange(2, 20) for _ in range(70 * 50 + 3)], D19, shuffled_tables(7), None, real,
                                      surplus)
    for groups in (1023, 1024, 1025):
        r = random.Random(groups)
        cases[f"sym-chunks-{groups}"] = _case([r.choice((2, 2, 3, 3, 4, 5)) for _ in range((groups - 1) * 50 + 49)], D19,
                                              [T_UP, T_DOWN], lambda g: (g // 5) % 2)
    r = random.Random(18001)
    cases["full-18001"] = _case([r.randrange(2, 20) for _ in range(MAX_N)], D19, shuffled_tables(8), lambda g: (5 * g + 1) % 6)
    return cases


def run_digits(count):
    digits = []
    bz2parse._flush_run(count, digits)
    return digits


def _mtf_cases():
    cases = {}
    for declared in (D19, D200):
        nd = len(declared)
        tag = f"@{nd}"
        tables = flat_tables(nd + 2)
        deepest = nd            # the symbol of the deepest position nd - 1

        # digit sequences of 1 .. 17 digits and of 19 (19 values) or 18 (200 values) -- all of 1 .. 19 exceed 900 000 bytes --
        # then short ones up to about 300 symbols; the digits of k are those of 2^k - 1 + (a few): mostly RUNA
        symbols = []
        lengths = list(range(1, 18)) + [19 if nd == 19 else 18] + [3, 1, 7, 2, 9, 1, 1, 4, 11, 2, 5, 3, 1, 2, 6, 2, 8]
        for i, k in enumerate(lengths):
            digits = [0] * k
            if k >= 3 and k < 17:
                digits[i % (k - 1)] = 1
            symbols += digits + [2 + (i * 5) % 18]       # shallow positions: the run bytes stay small, and so the payload
        cases["digits-across-chunks" + tag] = _case(symbols, declared, tables)

        # a run of c at every output position mod 16, c = 1 .. 40; literals in between
        symbols = []
        position = 0
        literal = 0
        for c in range(1, 41):
            for a in range(16):
                pad = (a - position) % 16 or 16
                for _ in range(pad):
                    symbols.append(2 + literal % (nd - 1))
                    literal += 7
                symbols += run_digits(c)
                position = (position + pad + c) % 16
        cases["runs-at-every-alignment" + tag] = _case(symbols, declared, tables)

        cases["run-first" + tag] = _case(run_digits(37) + [2, 3, deepest, 2] + run_digits(5) + [4] * 30, declared, tables)
        cases["run-900000" + tag] = _case(run_digits(MAX_N), declared, tables)
        cases["run-899999-literal" + tag] = _case(run_digits(MAX_N - 1) + [deepest], declared, tables)

        edges = [p for p in range(15, nd, 16) for p in (p, p + 1, p + 2) if p < nd]
        symbols = []
        for rounds in range(3):
            for p in edges:
                symbols += [p + 1, 2 + (p + rounds) % 3]
        symbols += [deepest] * 300 + run_digits(3) + [deepest] * 40
        cases["deep-positions" + tag] = _case(symbols, declared, tables)

    for nd in (128, 129):
        r = random.Random(nd)
        declared = list(range(64, 64 + nd))
        symbols = []
        for k in range(700):
            symbols += [nd] if k % 5 == 0 else ([r.randrange(2, nd + 1)] if k % 11 else run_digits(r.randrange(1, 70)))
        cases[f"count-{nd}"] = _case(symbols, declared, flat_tables(nd + 2))
    return cases


@functools.lru_cache(maxsize=None)
def _all_cases():
    scan, mtf = _scan_cases(), _mtf_cases()
    return scan, mtf


SCAN_NAMES = sorted(_all_cases()[0])
MTF_NAMES = sorted(_all_cases()[1])
NAMES = SCAN_NAMES + MTF_NAMES
SMALL_N = 70_000        # cases whose column is at most this long go into the large batch


def case(name):
    scan, mtf = _all_cases()
    return scan[name] if name in scan else mtf[name]


Model = collections.namedtuple("Model", "symbols declared column orig_ptr pre out crc stream group_starts selectors_written")


@functools.lru_cache(maxsize=None)
def model(name):
    """The case's stream and everything a decoder must find in it."""
    c = case(name)
    column = bz2parse.unmtf(c["symbols"], c["declared"])
    orig_ptr = (2 * len(column)) // 3
    pre, out, crc = crafted.model_decode(column, orig_ptr)
    stream, starts = bz2enc.encode_block_from_symbols(c["symbols"], c["declared"], orig_ptr, crc, c["tables"], c["selectors"],
                                                      c["selectors_written"])
    return Model(c["symbols"], c["declared"], column, orig_ptr, pre, out, crc, stream, starts, c["selectors_written"])


def column_length(name):
    """Bytes of the case's column, by its symbols alone."""
    symbols = case(name)["symbols"]
    return sum(1 for s in symbols[:-1] if s >= 2) + sum(bz2parse.zero_runs(symbols))


def small_names():
    return [name for name in NAMES if column_length(name) <= SMALL_N]


def big_names():
    return [name for name in NAMES if column_length(name) > SMALL_N]


@functools.lru_cache(maxsize=None)
def symbol_batch():
    """Every case with a column of at most SMALL_N bytes in one file and a shuffled list of (name, block bit offset) that
    names each block twice, 65 entries at least: the planner then gives k_mtf 512 lanes per block (more than 64 entries, at
    most 640).  Every stream is whole bytes long, so block k starts 32 bits into stream k."""
    names = small_names()
    data = bytearray()
    entries = []
    for name in names:
        entries.append((name, len(data) * 8 + 32))
        data += model(name).stream
    entries = entries * 2
    order = np.random.default_rng(0x5CA7).permutation(len(entries))
    entries = [entries[i] for i in order]
    assert 65 <= len(entries) <= 640
    return bytes(data), entries


# ---------------------------------------------------------------------------------------------------------------------
# what the scan is given: the selectors, every group's length in bits, where the symbols start
# ---------------------------------------------------------------------------------------------------------------------
ScanInput = collections.namedtuple("ScanInput", "sel n_sel glen p0 pos_base size_bits long_at eob_bit")


@functools.lru_cache(maxsize=None)
def scan_input(name):
    c = case(name)
    m = model(name)
    glen = []
    for g, t in enumerate(c["selectors"]):
        group = c["symbols"][g * GROUP_SYMS:(g + 1) * GROUP_SYMS]
        if g == len(c["selectors"]) - 1:
            group = group[:-1]                   # the last group's length: up to its end-of-block code
        glen.append(sum(c["tables"][t][s] for s in group))
    start = m.group_starts[0]
    pos_base = start & ~31
    assert [b - start for b in m.group_starts] == [0] + list(itertools.accumulate(glen))[:-1]
    # per table: at which absolute bit positions no code of up to SCAN_LUT_BITS bits starts (scan_build's pending list)
    bits = np.unpackbits(np.frombuffer(m.stream, dtype=np.uint8))
    padded = np.concatenate([bits, np.zeros(SCAN_MAX_SPAN + 64, dtype=np.uint8)]).astype(np.uint32)
    w10 = np.zeros(len(padded) - SCAN_LUT_BITS, dtype=np.uint32)
    for k in range(SCAN_LUT_BITS):
        w10 |= padded[k:k + len(w10)] << (SCAN_LUT_BITS - 1 - k)
    long_at = []
    for lengths in c["tables"]:
        short = np.zeros(1 << SCAN_LUT_BITS, dtype=bool)
        for l, code in zip(lengths, bz2enc.canonical_codes(lengths)):
            if l <= SCAN_LUT_BITS:
                short[code << (SCAN_LUT_BITS - l):(code + 1) << (SCAN_LUT_BITS - l)] = True
        long_at.append(~short[w10])
    eob_bit = start + sum(glen)
    return ScanInput(tuple(m.selectors_written), len(m.selectors_written), tuple(glen), start - pos_base, pos_base,
                     len(m.stream) * 8 - pos_base, long_at, eob_bit)


def scan_rows_per_wave(rows):
    """scan_rows_per_wave<1>: the builds are statically unrolled, the row count is rounded up to the next instance."""
    if rows <= 6:
        return min(rows, SCAN_ROWS)
    for instance in (8, 10, 12):
        if rows <= instance:
            return min(instance, SCAN_ROWS)
    return SCAN_ROWS


def _group_end(si, g, x, span):
    """Where the chase from offset x of a span of `span` positions ends for group g: an offset, OUT (a position at or behind
    the span) or TERM (the end-of-block code starts inside the span)."""
    end = x + si.glen[g]
    if end >= span:
        return OUT
    return TERM if g == len(si.glen) - 1 else end


def _pending(si, t, p, span, events):
    count = int(si.long_at[t][si.pos_base + p:si.pos_base + p + span].sum())
    if 2 * count > span:
        events["pending-over-half"] += 1
        if si.pos_base + p + span <= si.eob_bit:
            events["pending-over-half-in-mid-block"] += 1
            if span == SCAN_MAX_SPAN:
                events["pending-over-half-in-mid-block-full-span"] += 1


def _refill(p, w_hi, events):
    """Stream words up to (p + SCAN_MAX_SPAN + 64) >> 5, 64 at a time."""
    pieces = 0
    while (p >> 5) + (SCAN_MAX_SPAN + 96) // 32 > w_hi:
        w_hi += 64
        pieces += 1
    events["refills"] += pieces
    events["most-refills-at-once"] = max(events["most-refills-at-once"], pieces)
    return w_hi


def hscan_plan(si):
    """The loop of k_hscan<1> over the case's groups.  Returns (events, instances, left_at): counters of what happened, of
    the rows-per-build instances used, and of the chase index j at which a group left the span."""
    events, instances, left_at = collections.Counter(), collections.Counter(), collections.Counter()
    est = [0] * 6
    g, p, w_hi, force_full = 0, si.p0, 0, False
    starts = []
    while True:
        assert g < si.n_sel and g < MAX_SCAN_GROUPS
        w_hi = _refill(p, w_hi, events)
        t = si.sel[g]
        window_left = 64 - (g & 63)
        run = 1
        while g + run < si.n_sel and si.sel[g + run] == t:
            run += 1
        if run > window_left:
            events["run-clamped-at-window"] += 1
        run_len = min(run, window_left, si.n_sel - g, MAX_SCAN_GROUPS - g)
        near_end = p + SCAN_MAX_SPAN + 32 > si.size_bits
        rows, m = SCAN_ROWS, 1
        if est[t] != 0 and not force_full and not near_end:
            need = est[t] + (est[t] >> 3) + 16
            m = max(1, min((SCAN_MAX_SPAN - 24) // need, run_len))
            rows = min(SCAN_ROWS, (m * need + 24 + 63) >> 6)
        elif est[t] == 0:
            events["first-of-table"] += 1
        if force_full:
            events["full-after-leaving"] += 1
        force_full = False
        rw = SCAN_ROWS if near_end else scan_rows_per_wave(rows)
        span = 64 * rw
        events["near-end" if near_end else "builds"] += 1
        if not near_end:
            instances[rw] += 1
        events[f"m={m}"] += 1
        _pending(si, t, p, span, events)
        x, done, stop = 0, 0, False
        for j in range(m):
            u = _group_end(si, g + j, x, span)
            if u == OUT:
                force_full = j == 0
                left_at[j] += 1
                break
            starts.append(p + x)
            if (g + j) & 63 == 63:
                events["window-written"] += 1
            done += 1
            if u == TERM:
                stop = True
                break
            d = u - x
            est[t] = d if est[t] == 0 or d > est[t] else est[t] - ((est[t] - d) >> 2)
            x = u
        g += done
        p += x
        assert done > 0 or force_full
        if stop:
            break
    events["tail-partial" if g & 63 else "tail-empty"] += 1
    assert starts == [si.p0 + a for a in [0] + list(itertools.accumulate(si.glen))[:-1]]
    events["groups"] = g
    return events, instances, left_at


def spec_plan(si, K):
    """The unit loop of k_hscan_spec<K>.  Returns a counter of what happened: which term of `ok` cut a unit ("cut-..."), how
    the chain ended ("chain-..."), windows taken from the next 64 selectors, ring refills."""
    events = collections.Counter()
    est, mid, dev = [0] * 6, [0] * 6, [0] * 6
    g, p, w_hi, force_full = 0, si.p0, 0, False
    n_groups = len(si.glen)
    while True:
        assert g < si.n_sel and g < MAX_SCAN_GROUPS
        plan = []                      # (table, lo, width, rows) of the usable slots
        acc_lo = acc_hi = 0
        cut = "all-slots"
        for w in range(K):
            gw = g + w
            if gw >= si.n_sel:
                cut = "selectors"
                break
            if gw >= MAX_SCAN_GROUPS:
                cut = "max-groups"
                break
            t = si.sel[gw]
            need = est[t] + (est[t] >> 3) + 16
            slack = dev[t] + (dev[t] >> 2) + 2
            step_lo = mid[t] - slack if mid[t] > slack + 50 else 50
            step_hi = mid[t] + slack
            width = acc_hi - acc_lo
            if est[t] == 0:
                cut = "table-not-seen"
                break
            if width + need + 24 > SCAN_MAX_SPAN:
                cut = "span"
                break
            if acc_hi > SPEC_REACH:
                cut = "reach"
                break
            if p + acc_lo + SCAN_MAX_SPAN + 32 > si.size_bits:
                cut = "near-end"
                break
            plan.append((t, acc_lo, width, scan_rows_per_wave((width + need + 24 + 63) >> 6), (gw >> 6) != (g >> 6)))
            acc_lo += step_lo
            acc_hi += step_hi
            if step_lo == 50:
                events["step-lo-floor"] += 1
        events["cut-" + cut] += 1
        if force_full:
            plan = []
            events["full-after-0xffff"] += 1
        full = not plan
        near_end = p + SCAN_MAX_SPAN + 32 > si.size_bits
        if full:
            plan = [(si.sel[g], 0, 0, SCAN_ROWS, False)]
            events["full-units"] += 1
            if near_end:
                events["near-end-units"] += 1
        events[f"n={len(plan)}"] += 1
        events["from-next-window"] += sum(1 for slot in plan if slot[4])
        # stream words up to the end of the farthest build
        pieces = 0
        while ((p + plan[-1][1]) >> 5) + (SCAN_MAX_SPAN + 96) // 32 > w_hi:
            w_hi += 64
            pieces += 1
        events["refills"] += pieces
        events["most-refills-at-once"] = max(events["most-refills-at-once"], pieces)
        for t, lo, width, rows, _ in plan:
            _pending(si, t, p + lo, 64 * rows, events)
            assert (width >> 6) + 1 <= rows
        # the chain
        rel, measured, last = 0, 0, None
        lengths = []
        while measured < len(plan):
            t, lo, width, rows, _ = plan[measured]
            y = rel - lo
            if y < 0 or y > width:
                last = "stray"
                assert measured > 0
                break
            u = _group_end(si, g + measured, y, 64 * rows)
            if u in (OUT, TERM):
                last = u
                break
            lengths.append((t, u - y))
            rel = lo + u
            measured += 1
        force_full = last == OUT and measured == 0
        stop = last == TERM
        if last == OUT:
            events["chain-0xffff-at-slot-0" if measured == 0 else "chain-0xffff-later"] += 1
        elif last == "stray":
            events["chain-stray"] += 1
        elif last == TERM:
            events["chain-terminal"] += 1
        else:
            events["chain-complete"] += 1
        done = measured + (1 if stop else 0)
        assert done > 0 or force_full
        if done >= 64 - (g & 63):
            events["window-written"] += 1
        for t in range(6):
            mine = [d for tw, d in lengths if tw == t]
            if not mine:
                continue
            d_max, d_min = max(mine), min(mine)
            first = est[t] == 0
            mid_old = d_max if first else mid[t]
            off = max(abs(d_max - mid_old), abs(d_min - mid_old))
            centre = (d_max + d_min) >> 1
            est[t] = d_max if first or d_max > est[t] else est[t] - ((est[t] - d_max) >> 2)
            half = abs(centre - mid[t]) // 2                       # C++ division truncates towards zero
            mid[t] = d_max if first else mid[t] + (half if centre >= mid[t] else -half)
            dev[t] = (d_max >> 3) + 8 if first else (off if off > dev[t] else dev[t] - ((dev[t] - off + 3) >> 2))
        g += done
        p += rel
        if stop:
            break
    assert g == n_groups and p == si.p0 + sum(si.glen[:-1])      # p stays at the start of the terminal group
    events["tail-partial" if g & 63 else "tail-empty"] += 1
    return events


def selectable_instances():
    """Every rows-per-build instance that k_hscan<1>'s rule can select for groups of 50 .. 1 000 bits: est is a group
    length, m any count the rule allows."""
    found = set()
    for est in range(GROUP_SYMS, 20 * GROUP_SYMS + 1):
        need = est + (est >> 3) + 16
        for m in range(1, max(1, (SCAN_MAX_SPAN - 24) // need) + 1):
            found.add(scan_rows_per_wave(min(SCAN_ROWS, (m * need + 24 + 63) >> 6)))
    return found


def selector_plan(name):
    """scan_parse's selector pass over the case's stream: rounds of 2 048 bits from the cursor, every zero ends a code.
    Returns (rounds, whether a round took fewer codes than it saw, the ones carried across the 32-bit words of taken
    codes, the header bits the selectors take)."""
    m = model(name)
    n_sel = len(m.selectors_written)
    rows = len({b >> 4 for b in m.declared})
    cursor = 32 + 48 + 32 + 1 + 24 + 16 + 16 * rows + 3 + 15
    first = cursor
    bits = np.unpackbits(np.frombuffer(m.stream, dtype=np.uint8)).tolist() + [0] * 4096
    done, rounds, short_take, carries = 0, 0, False, set()
    while done < n_sel:
        window = bits[cursor:cursor + 2048]
        zeros = [i for i, b in enumerate(window) if b == 0]
        take = min(len(zeros), n_sel - done)
        assert take > 0
        short_take |= take < len(zeros)
        previous = -1
        for z in zeros[:take]:
            start = previous + 1
            if start // 32 != z // 32:
                carries.add(32 * (z // 32) - start)
            previous = z
        cursor += zeros[take - 1] + 1
        done += take
        rounds += 1
    return rounds, short_take, carries, cursor - first


# ---------------------------------------------------------------------------------------------------------------------
# k_mtf
# ---------------------------------------------------------------------------------------------------------------------
def mtf_lanes(declared_count, batch_entries, narrow=False):
    """Lanes per block of k_mtf: planBatch's mtfSmallLanes for the 144 stride, 512 or 256 for the 272 stride."""
    small = 256
    if batch_entries <= 640 and not narrow:
        small = 1024 if batch_entries <= 64 else 512
    if declared_count <= MTF_SMALL_ENTRIES:
        return small
    return 512 if small > 256 else 256


def mtf_chunks(symbols, lanes):
    """Where every lane's chunk of `symbols` (without the end of block) begins: never inside a digit sequence."""
    n = len(symbols)
    step = -(-n // lanes) if n else 0
    starts = []
    for t in range(lanes):
        begin = min(t * step, n)
        while 0 < begin < n and symbols[begin] <= 1 and symbols[begin - 1] <= 1:
            begin += 1
        starts.append(begin)
    return starts + [n]


def mtf_lane_of(symbols, lanes, index):
    """The lane whose chunk holds symbol `index`."""
    starts = mtf_chunks(symbols, lanes)
    for t in range(lanes):
        if starts[t] <= index < starts[t + 1]:
            return t
    return lanes - 1


def _sink_fill(o, count, events):
    """ByteSink::fill by its branches; returns the new position."""
    n = o & 3
    if n:
        take = min(count, 4 - n)
        events["fill-head-short" if take < 4 - n else "fill-head-full"] += 1
        o += take
        count -= take
    while count >= 4 and o & 15:
        events["fill-lead-dword"] += 1
        o += 4
        count -= 4
    if count >= 16:
        events["fill-units"] += 1
        o += count & ~15
        count &= 15
    while count >= 4:
        events["fill-tail-dword"] += 1
        o += 4
        count -= 4
    if count:
        events["fill-tail-bytes"] += 1
    return o + count


FILL_BRANCHES = ("fill-head-short", "fill-head-full", "fill-lead-dword", "fill-units", "fill-tail-dword", "fill-tail-bytes")


def mtf_plan(symbols, lanes):
    """k_mtf's chunk rule and pass B's byte sink over `symbols` (without the end of block).  Returns (events, alignments):
    counters of chunk shapes and fill branches, and the set of (output position mod 16, run length) of all runs."""
    events = collections.Counter()
    starts = mtf_chunks(symbols, lanes)
    n = len(symbols)
    step = -(-n // lanes) if n else 0
    alignments = set()
    o = 0
    for t in range(lanes):
        begin, end = starts[t], starts[t + 1]
        if begin == end:
            events["empty-chunks"] += 1
        if begin != min(t * step, n):
            events["pushed-chunks"] += 1
        if t and begin == starts[t - 1] and begin < n:
            events["same-begin"] += 1
        lo = o
        run, weight = 0, 1
        for s in symbols[begin:end]:
            if s <= 1:
                run += weight << s
                weight <<= 1
                continue
            if run:
                alignments.add((o & 15, run))
                if o + run == MAX_N:
                    events["run-ends-at-max-n"] += 1
                o = _sink_fill(o, run, events)
                run, weight = 0, 1
            if o == MAX_N - 1:
                events["literal-at-the-last-byte"] += 1
            o += 1
        if run:
            alignments.add((o & 15, run))
            if o + run == MAX_N:
                events["run-ends-at-max-n"] += 1
            if begin == 0 and all(s <= 1 for s in symbols[begin:end]):
                events["chunk-is-one-run"] += 1
            o = _sink_fill(o, run, events)
        if (lo & 15) and o > lo:
            events["head-shared-with-previous-lane"] += 1
        if (o & 15) and o > lo:
            events["tail-shared-with-next-lane"] += 1
    events["bytes"] = o
    return events, alignments
