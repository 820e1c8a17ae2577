#!/usr/bin/env python3
"""G16: SHA-256 digests and sizes of everything FcnEngine hands to the library, for the cases of tests/test_fcn_packing_identity.py
(whose recording proxy and case table this script runs).  CPU only: the emulated library of tests/hipemu stands behind the proxy.
The file pins the host side's packing: regenerate it only with a change that means to alter what is packed, never with a refactor.

  python tests/golden/make_golden_fcn_packing.py [--dump DIR]      (--dump: also the per-call log of every case, one JSON file each)
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import test_fcn_packing_identity as ident  # noqa: E402
from lecturemath_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    args = ap.parse_args()
    emu = os.path.join(TESTS, "hipemu")
    subprocess.check_call(["make", "-s", "-C", emu])
    lib = _lib.load(os.path.join(emu, "liblecturemath_emu.so"))
    cases = {}
    for name in ident.CASES:
        cases[name], calls = ident.run_case(lib, name)
        print(name, cases[name]["calls"], "calls", cases[name]["bytes"], "bytes", cases[name]["sha256"][:16])
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + ".json"), "w") as f:
                json.dump(calls, f, indent=1)
    with open(ident.GOLDEN_JSON, "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
