"""Writes tests/golden/blake3_long.json: the oracle's BLAKE3 (oracle/pyref.py, pinned to the published vectors at 0, 1 and 1025 by
tests/test_oracle.py) of the published test input -- byte i = i mod 251 -- at the lengths of BLAKE3's published vector file plus the
block edges below 128.  ~250 KB of input, about half a second:   python tests/golden/gen_blake3_long.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

import pyref as o  # noqa: E402

LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169,
           8192, 8193, 16384, 31744, 102400]

if __name__ == "__main__":
    out = {str(n): o.blake3(bytes(i % 251 for i in range(n))).hex() for n in LENGTHS}
    with open(os.path.join(HERE, "blake3_long.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
