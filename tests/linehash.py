"""A plain Python model of the line hash (indexed_bzip2_amd/csrc/bz2_linehash.hpp): the hash itself, the summary of a
stretch, the summary of a stretch cut into chunks, and the rule that stitches stretches that lie back to back.  Python's
integers do the arithmetic; nothing here calls the code under test."""

P = 2**61 - 1
MASK = 2**64 - 1


def splitmix64(s):
    z = (s + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def base(seed):
    return 256 + splitmix64(seed) % (P - 256)


def line_hash(content, seed=0):
    x, h = base(seed), 0
    for b in content:
        h = (h * x + b + 1) % P
    return h


def part(content, x):
    """(h, xl) of a byte string."""
    h = 0
    for b in content:
        h = (h * x + b + 1) % P
    return h, pow(x, len(content), P)


def followed_by(a, b):
    return (a[0] * b[1] + b[0]) % P, a[1] * b[1] % P


def lines_of(data, nl):
    """The contents of the lines of data as grep numbers them: a non-empty unterminated tail is one more line."""
    pieces = bytes(data).split(bytes([nl]))
    return pieces[:-1] + ([pieces[-1]] if pieces[-1] else [])


def direct(data, nl, seed=0):
    """The hash of every line of data, by the definition."""
    return [line_hash(content, seed) for content in lines_of(data, nl)]


def summarise_chunk(data, nl, x):
    """The summary of one stretch, walked byte by byte: a dict with head, tail (each (h, xl)), has_delimiter,
    tail_non_empty and hashes (of the lines it closes, the first as if entered with hash 0)."""
    data = bytes(data)
    pieces = data.split(bytes([nl]))
    summary = {"head": part(pieces[0], x), "has_delimiter": len(pieces) > 1, "tail": (0, 1),
               "tail_non_empty": len(data) > 0 and data[-1] != nl, "hashes": [part(c, x)[0] for c in pieces[:-1]]}
    if len(pieces) > 1:
        summary["tail"] = part(pieces[-1], x)
    return summary


def append(left, right):
    """left followed by right, both summaries."""
    carry = left["tail"] if left["has_delimiter"] else left["head"]
    out = dict(left, hashes=list(left["hashes"]))
    if right["has_delimiter"]:
        out["hashes"].append(followed_by(carry, right["head"])[0])
        out["hashes"] += right["hashes"][1:]
        if not left["has_delimiter"]:
            out["head"] = followed_by(left["head"], right["head"])
        out["tail"] = right["tail"]
        out["has_delimiter"] = True
        out["tail_non_empty"] = right["tail_non_empty"]
    else:
        joined = followed_by(carry, right["head"])
        out["tail" if left["has_delimiter"] else "head"] = joined
        out["tail_non_empty"] = left["tail_non_empty"] or right["tail_non_empty"]
    return out


EMPTY = {"head": (0, 1), "has_delimiter": False, "tail": (0, 1), "tail_non_empty": False, "hashes": []}


def summarise(data, nl, x, chunk):
    """The summary of data, cut into chunks of `chunk` bytes and composed."""
    out = EMPTY
    for at in range(0, len(data), chunk):
        out = append(out, summarise_chunk(data[at:at + chunk], nl, x))
    return out


def stitch(summaries):
    """The hashes of all lines of stretches that lie back to back from offset 0 to the end of the file, from their
    summaries alone: a carry that starts at (0, 1); with a delimiter the first closed line becomes carry.h * head.xl +
    head.h and the carry becomes the tail; without one the carry becomes the carry followed by the head; at the end a
    carry over at least one byte is the unterminated tail."""
    hashes, carry, non_empty = [], (0, 1), False
    for s in summaries:
        if s["has_delimiter"]:
            hashes.append((carry[0] * s["head"][1] + s["head"][0]) % P)
            hashes += s["hashes"][1:]
            carry, non_empty = s["tail"], s["tail_non_empty"]
        else:
            carry = followed_by(carry, s["head"])
            non_empty = non_empty or s["tail_non_empty"]
    if non_empty:
        hashes.append(carry[0])
    return hashes


class Prefix:
    """The hashes of all prefixes of one byte string, computed once, so that a test over many spans of the same text
    pays for the text once: part(a, b) is part(data[a:b], x), by H[b] - H[a] * x^(b - a)."""

    def __init__(self, data, x):
        self.data, self.x = bytes(data), x
        self.h = [0] * (len(self.data) + 1)
        h = 0
        for i, b in enumerate(self.data):
            h = (h * x + b + 1) % P
            self.h[i + 1] = h

    def part(self, a, b):
        xl = pow(self.x, b - a, P)
        return (self.h[b] - self.h[a] * xl) % P, xl

    def summary(self, offset, size, nl):
        """summarise_chunk(data[offset:offset + size], nl, x)."""
        end = offset + size
        cuts, at = [], self.data.find(bytes([nl]), offset, end)
        while at >= 0:
            cuts.append(at)
            at = self.data.find(bytes([nl]), at + 1, end)
        starts = [offset] + [c + 1 for c in cuts]
        summary = {"head": self.part(offset, cuts[0] if cuts else end), "has_delimiter": bool(cuts), "tail": (0, 1),
                   "tail_non_empty": size > 0 and self.data[end - 1] != nl,
                   "hashes": [self.part(a, b)[0] for a, b in zip(starts, cuts)]}
        if cuts:
            summary["tail"] = self.part(cuts[-1] + 1, end)
        return summary

    def lines(self, nl):
        """direct(data, nl, seed) for the seed of x."""
        summary = self.summary(0, len(self.data), nl)
        tail = [summary["tail" if summary["has_delimiter"] else "head"][0]] if summary["tail_non_empty"] else []
        return summary["hashes"] + tail
