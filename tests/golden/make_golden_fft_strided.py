#!/usr/bin/env python3
"""Record tests/golden/fft_strided_before.json: the SHA-256 of the raw float32 bytes of every result of
tests/fft_strided_cases.py (and its first eight values, only so that a mismatch can be read), on an MI355X.

    python tests/golden/make_golden_fft_strided.py [output.json]

Run ONCE, with the code and the library of the commit BEFORE the strided FFT refactor: the file is that commit's answer,
which tests/test_gpu_fft_strided_bits.py holds every later commit to.  Do not regenerate it to make a test pass.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.fft_strided_cases import CASES, digest, run    # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fft_strided_before.json")
    rec = {}
    for name in CASES:
        rec[name] = digest(run(name))
        print(name, rec[name]["sha256"][:16], flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(rec), "cases")


if __name__ == "__main__":
    main()
