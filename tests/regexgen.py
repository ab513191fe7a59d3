"""What the regular-expression tests share: the pattern lists, Python's `re` as the reference for which lines match, and
a model of the summaries (bz2_regex.hpp: summarise and stitchSummaries) that drives a compiled table.

The model mirrors the rule, not the code: a chunk's head is run for every entry state, its body once from state 0; chunks
compose into a stretch, stretches into a file.  The host tests drive it with the table of compile_regex and compare with
`re`; the device tests predict with it what match_lines must return for a span."""
import random
import re

START, MATCHED = 0, 1

# every accepted construct at least once; all compile within 64 states (test_regex_plan checks that none is skipped)
FIXED_PATTERNS = [
    rb"error",
    rb"a*",
    rb"^$",
    rb"a^b",
    rb"$a",
    rb"(^|,)x(,|$)",
    rb"[^a]",
    rb"\xe9t\xe9",
    rb"[\x80-\xff]+",
    rb"a{,2}b",
    rb"^a+$",
    rb"x.*y.*z",
    rb"(error|warning|fatal)",
    rb"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}",
    rb"^(GET|POST) /[a-z/]* HTTP/1\.[01]$",
    rb"^[0-9]{4}-[0-9]{2}-[0-9]{2} .*(ERROR|FATAL)",
    rb"\.$",
    rb"^.$",
    rb"^\s*$",
    rb"\w+@\w+\.com",
    rb"\D\d\D",
    rb"\W\w\W",
    rb"\S\s\S",
    rb"[a-c]{3}",
    rb"[^a-c\n]{2,}$",
    rb"(?:ab)+c",
    rb"(ab|cd)*ef",
    rb"a?b?c?d",
    rb"a+b+",
    rb"a{2}",
    rb"a{2,}b",
    rb"a{1,3}c",
    rb"[\d\s]x",
    rb"[\w.-]+:",
    rb"[a\-c]b",
    rb"[\]\[]",
    rb"\(\)|\[\]|\{\}",
    rb"\t|\r|\f|\v|\0",
    rb"q|",
    rb"(|a)b",
    rb"^(a|b)*c",
    rb"}x|]y",
    rb"^a|b$",
    rb"(a$|^b)c?",
    rb"dolor(em)?[ ,.]",
    rb"[Qq]u[aeiou]+",
    rb"^\S+ \S+$",
    rb".\x00.",
]

# (pattern, the word the error message must hold)
REFUSED = [
    (rb"(a)\1", "back-reference"),
    (rb"a(?=b)", "look-around"),
    (rb"a(?!b)", "look-around"),
    (rb"(?<=a)b", "look-around"),
    (rb"(?<!a)b", "look-around"),
    (rb"(?i)a", "inline flags"),
    (rb"(?s:a)", "inline flags"),
    (rb"(?P<x>a)", "named group"),
    (rb"(?P=x)", "named group"),
    (rb"a*?", "lazy"),
    (rb"a+?", "lazy"),
    (rb"a??", "lazy"),
    (rb"a{1,2}?", "lazy"),
    (rb"a*+", "possessive"),
    (rb"a++", "possessive"),
    (rb"a\b", "\\b"),
    (rb"a\B", "\\B"),
    (rb"\Aa", "\\A"),
    (rb"a\Z", "\\Z"),
    (rb"", "empty pattern"),
    (b"a" * 4097, "4096"),
    (rb"a{256}", "255"),
    (rb"a{3,2}", "min above max"),
    (rb"a{", "'{'"),
    (rb"a{x}", "'{'"),
    (rb"{1}", "'{'"),
    (rb"*a", "nothing to repeat"),
    (rb"(|*)", "nothing to repeat"),
    (rb"^*", "nothing to repeat"),
    (rb"a**", "multiple repeat"),
    (rb"(a", "unbalanced"),
    (rb"a)", "unbalanced"),
    (rb"[a", "unterminated class"),
    (rb"[]a]", "']'"),
    (rb"[z-a]", "range"),
    (rb"[\d-z]", "range"),
    (rb"\012", "octal"),
    (rb"\x4", "\\xHH"),
    (rb"\q", "escape \\q"),
    (rb"[\b]", "escape \\b"),
    (b"a\\", "backslash"),
    (rb"(?#c)a", "comment"),
    (rb"(?>a)", "atomic"),
]


def random_pattern(rng, depth=0):
    """A pattern from a small grammar over the alphabet of random_corpus; most compile to a handful of states."""
    def atom():
        kind = rng.randrange(10)
        if kind < 4:
            return rng.choice([b"a", b"b", b"c", b",", b" "])
        if kind == 4:
            return b"."
        if kind == 5:
            return rng.choice([b"[ab]", b"[^a]", b"[a-c]", b"[^bc ]", b"\\w", b"\\s", b"\\S", b"\\d", b"\\D"])
        if kind == 6 and depth < 2:
            return b"(" + random_pattern(rng, depth + 1) + b")"
        if kind == 7 and depth < 2:
            return b"(?:" + random_pattern(rng, depth + 1) + b"|" + random_pattern(rng, depth + 1) + b")"
        return rng.choice([b"a", b"b", b"1"])

    parts = []
    if rng.randrange(5) == 0:
        parts.append(b"^")
    for _ in range(rng.randrange(1, 4)):
        piece = atom()
        quantifier = rng.randrange(9)
        if quantifier < 5:
            piece += [b"*", b"+", b"?", b"{2}", b"{1,2}"][quantifier] if quantifier < 3 or depth == 0 else b""
        parts.append(piece)
    if rng.randrange(5) == 0:
        parts.append(b"$")
    return b"".join(parts)


def random_corpus(seed, lines=400):
    """Lines over a small alphabet, empty ones and repeats included, without the delimiter."""
    rng = random.Random(seed)
    out = []
    for _ in range(lines):
        out.append(bytes(rng.choice(b"aabbc, 1A\t") for _ in range(rng.choice([0, 1, 1, 2, 3, 5, 8, 13]))))
    return out


def split_lines(data, nl=b"\n"):
    """[(offset, content)] of the lines of `data`: the unterminated tail is a line only if it is non-empty."""
    lines, at = [], 0
    while at < len(data):
        end = data.find(nl, at)
        if end < 0:
            lines.append((at, data[at:]))
            break
        lines.append((at, data[at:end]))
        at = end + 1
    return lines


def reference_flags(ignore_case):
    return re.DOTALL | (re.IGNORECASE if ignore_case else 0)


def expected_lines(pattern, data, nl=b"\n", ignore_case=False):
    """The 0-based numbers of the lines of `data` that Python's re finds a match in."""
    compiled = re.compile(pattern, reference_flags(ignore_case))
    return [k for k, (_, content) in enumerate(split_lines(data, nl)) if compiled.search(content)]


def table_matches(transitions, accepts, content):
    """Run the table over one line's content."""
    state = START
    for byte in content:
        state = int(transitions[state][byte])
        if state == MATCHED:
            return True
    return bool(accepts[state])


class Summary:
    def __init__(self, n):
        self.head_map = list(range(n))
        self.has_delimiter = False
        self.exit = 0
        self.witnesses = []

    def padded_head_map(self):
        return self.head_map + [0] * (64 - len(self.head_map))


def chunk_summary(transitions, accepts, data, nl, base=0):
    n = len(accepts)
    s = Summary(n)
    at = 0
    while at < len(data) and data[at] != nl:
        s.head_map = [int(transitions[q][data[at]]) for q in s.head_map]
        at += 1
    if at == len(data):
        return s
    s.has_delimiter = True
    state = START
    for at in range(at + 1, len(data)):
        byte = data[at]
        if byte == nl:
            if state != MATCHED and accepts[state]:
                s.witnesses.append(base + at)
            state = START
            continue
        following = int(transitions[state][byte])
        if following == MATCHED and state != MATCHED:
            s.witnesses.append(base + at)
        state = following
    s.exit = state
    return s


def head_line_matches(accepts, summary, entry):
    if entry == MATCHED:
        return False
    behind = summary.head_map[entry]
    return behind == MATCHED or (summary.has_delimiter and bool(accepts[behind]))


def summarise(transitions, accepts, data, nl, chunk, base=0):
    """The summary of `data` cut into chunks of `chunk` bytes; nl is the delimiter's byte value."""
    n = len(accepts)
    total = Summary(n)
    for at in range(0, len(data), chunk):
        part = chunk_summary(transitions, accepts, data[at:at + chunk], nl, base + at)
        if total.has_delimiter:
            if head_line_matches(accepts, part, total.exit):
                total.witnesses.append(base + at)
            total.exit = part.exit if part.has_delimiter else part.head_map[total.exit]
        else:
            total.head_map = [part.head_map[q] for q in total.head_map]
            total.has_delimiter = part.has_delimiter
            total.exit = part.exit
        total.witnesses += part.witnesses
    return total


def stitch(accepts, stretches):
    """stretches: [(offset, size, Summary)] back to back from 0 -> one offset inside every matching line, ascending."""
    witnesses, entry, end = [], START, 0
    for offset, size, summary in stretches:
        assert offset == end
        end += size
        if size == 0:
            continue
        if head_line_matches(accepts, summary, entry):
            witnesses.append(offset)
        witnesses += summary.witnesses
        entry = summary.exit if summary.has_delimiter else summary.head_map[entry]
    if entry not in (START, MATCHED) and accepts[entry]:
        witnesses.append(end - 1)
    return witnesses


def lines_of_offsets(data, offsets, nl=b"\n"):
    """The 0-based number of the line that holds each offset."""
    return [data.count(nl, 0, p) for p in offsets]
