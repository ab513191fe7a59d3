"""Generate tests/golden/crafted_symbols_vectors.json from the REAL reference (oracle/_ref/ref_bz2 probe), in the manner of
make_golden_crafted.py: for every crafted symbol stream (tests/crafted_symbols.py), full-18001 and the 900 000-byte runs
included, the sha256 of its stream and what the reference's probe says about the block at bit 32 -- verdict, encoded
size, header and calculated CRC, decoded size and the FNV-64 of the decoded bytes.  Data only; the streams are reproducible
from tests/crafted_symbols.py + tests/bz2enc.py."""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import crafted
import crafted_symbols
from oracle import oracle as O

OUT = os.path.join(ROOT, "tests", "golden", "crafted_symbols_vectors.json")


def main():
    assert O.ref_available(), "build oracle/_ref first: make -C oracle ref"
    cases = {}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "case.bz2")
        for name in crafted_symbols.NAMES:
            enc = crafted_symbols.model(name).stream
            with open(path, "wb") as f:
                f.write(enc)
            cases[name] = dict(crafted.parse_probe(O.ref_run("probe", path, 32)), enc_sha256=hashlib.sha256(enc).hexdigest())
    with open(OUT, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", sum(c["verdict"] == "OK" for c in cases.values()), "of", len(cases), "OK")


if __name__ == "__main__":
    main()
