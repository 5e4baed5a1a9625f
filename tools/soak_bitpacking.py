#!/usr/bin/env python3
"""Soak of the BITPACKING path: random columns from the in-suite fuzz's generator (type, length, per-group value
patterns over the whole range, NULLs, forced modes) compressed by the oracle's restatement of the reference and by
the device; refusals must agree, block images must be byte-identical, the device decode (full, ranged, point fetch)
must return the original rows.
usage: python tools/soak_bitpacking.py [first_seed] [count]"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_bitpacking_fuzz as fz  # noqa: E402

adac = importlib.import_module("duckdb-adaptive-compression_amd")
adac.build()
ctx = adac.Context(0)


def one(seed):
    """the in-suite fuzz's generator and checks (tests/test_gpu_bitpacking_fuzz.py), one seed"""
    fz.check_seed(adac, ctx, seed)


first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
count = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
bad = []
for seed in range(first, first + count):
    try:
        one(seed)
    except Exception as e:  # noqa: BLE001
        bad.append((seed, repr(e)[:300]))
        if len(bad) >= 5:
            break
    if (seed - first) % 200 == 199:
        print("seed", seed, "failures so far", len(bad), flush=True)
print("done: %d seeds, %d failures" % (count, len(bad)))
for b in bad:
    print(b)
sys.exit(1 if bad else 0)
