"""indexed_bzip2_amd -- MI355X-native parallel bzip2 block decoder behind the indexed_bzip2 API, and a GPU encoder
(compress, compress_many).

Host-side mirror of python/indexed_bzip2/indexed_bzip2.pyx (open, IndexedBzip2File, ...) over the C ABI of
include/mi355x_bz2.h.  All decoding happens in hand-written HIP kernels on gfx950; there is no CPU fallback.

Beyond the reference's API the reader answers questions about the decoded file while its bytes stay in HBM: byte ranges
(read_ranges), lines (count_lines, line_starts, line_numbers, read_line_ranges), where a byte string occurs
(count_matches, find_all, find: every offset p with data[p:p + len(pattern)] == pattern, overlapping occurrences included)
and which lines hold it (grep, count_matching_lines, grep_to_tensor: the lines of the matches' first bytes, each once,
whole, with their 0-based numbers).  The same for a set of up to 1 024 byte strings with one decode of the file per call
(count_matches_each, find_all_any, find_any, grep_any, count_matching_lines_any, grep_any_to_tensor).  Every one of these
search and grep methods takes the keyword-only ignore_case=True, which folds the ASCII letters of pattern and data on the
GPU (bytes.lower() on both sides, `LC_ALL=C grep -i`; the bytes 0x80 to 0xFF are never folded).  And the lines that match
a regular expression (grep_regex, count_matching_lines_regex, grep_regex_to_tensor): compile_regex turns a subset of
Python's bytes `re` syntax into a DFA of at most 64 states on the host, and the GPU runs it over the decoded file.  And
which lines are the same: line_hashes and line_hashes_to_tensor give one 61-bit polynomial hash per line (line_hash says
which, and computes it on the CPU), count_distinct_lines and first_occurrences sort them on the GPU (`sort -u | wc -l`,
`awk '!seen[$0]++'`).  Distinct lines have distinct hashes with overwhelming probability, not with certainty: two contents
of at most L bytes collide for at most L of the 2^61 bases a seed selects, and a second seed is an independent check.
And what a line holds: field_spans and field_spans_to_tensor say where field j of every line lies when the line is split at
a delimiter byte exactly as bytes.split splits it (size -1 where a line has fewer fields), read_fields and
read_fields_to_tensor bring those bytes and nothing else (`cut -f`, `awk -F`); there is no quoting or escaping, this is not
a CSV parser -- unless quote=b'"' is given to field_spans, read_fields or read_columns: then a delimiter inside quotes does
not split the line and a field comes back without its enclosing pair of quotes (doubled quotes inside stay doubled, and a
newline still ends every line).  And how often each value of a column occurs: field_hashes and field_hashes_to_tensor give the hash of
field j of every line (FIELD_MISSING, 2^61 - 1, where a line has no such field), count_by_field groups the lines by it on
the GPU and value_counts adds the values (`cut -f3 | sort | uniq -c | sort -rn`).  And how much: field_ints and
field_ints_to_tensor give field j of every line as an int64 (parse_field_number says which bytes are a number:
[+-]?[0-9]{1,18}, not awk's strtod; FIELD_NOT_A_NUMBER and FIELD_NUMBER_MISSING otherwise), sum_by_field sums one column
per value of another on the GPU from one decode, exactly, and value_sums adds the keys (`awk '{s[$1]+=$3}'`).  And which
rows: where_field, where_field_to_tensor and count_where_field select the lines whose field j is byte for byte one of a set
of values, or whose number lies in a range (`awk -F'\t' '$3 == "GET"'`, `awk '$5 >= 500'`, a semi-join), or, with
regex=pattern, whose field matches a regular expression of grep_regex's kind, anchored to the field's ends (`awk -F'\t'
'$3 ~ /^GET$/'`), invert=True the others; select_lines and select_lines_to_tensor bring those lines as grep brings its own.
"""
__version__ = "0.1.0"

import os as _os

# the reader drives two or three decoder contexts with up to eight HIP streams each (block groups, input, copy-out): the
# runtime's default of 4 hardware queues serialises them.  Measured: the bench (four contexts, 2 560 blocks per batch) 85.8 ms
# per step with 8 queues, 67 with 16 or more; batches of 310 blocks on four contexts 12.4 ms per step with 16 queues but 17.3
# with 24 or 32.  The HIP runtime reads this when it starts, so it only helps if nothing has touched the GPU yet; an
# existing setting wins
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

from ._native import (FIELD_MISSING, FIELD_NOT_A_NUMBER, FIELD_NUMBER_MISSING, Bz2Error, CompiledRegex, Decoder,  # noqa: F401
                      compile_regex, find_magic, lib, line_hash, parse_field_number, plan_compress_blocks, status_string, warmup)
from .buffers import (compress, compress_many, decompress, decompress_many,  # noqa: F401
                      decompress_many_to_tensor)
from .reader import (IndexedBzip2File, IndexedBzip2FileRaw, open, read_block_offsets,  # noqa: F401
                     read_line_offsets, write_block_offsets, write_line_offsets)

if _os.environ.get("MI355X_BZ2_WARMUP") == "1":     # opt-in: see warmup()
    warmup()
