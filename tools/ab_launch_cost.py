#!/usr/bin/env python3
"""Host cost per call of the scan entry points between library builds, in ONE process on ONE box: a layout small enough
(one segment, 1024 rows) that the launch path dominates, `--calls` back-to-back calls followed by one sync, wall time
per call; and, because such a sequence can be bound by the device running the calls' kernels rather than by the host
path, the host time alone (`host_only`): bursts of `--burst` calls enqueued on an idle stream, timed up to the last
call's return.  Every library is loaded as a binding of its own (the same build under two file names gives two
separate copies: their difference is the run-to-run margin), the libraries take every place in a round in turn and the
median of the rounds is kept.  The outputs of every library are compared with the first one's.

The binding created last (`--new`) has come out 0.2 - 0.4 us per call slower back to back whichever library it holds
(profiles/r14_launch_layer.json), so a second run with the libraries' places exchanged belongs to every comparison.

  python tools/ab_launch_cost.py --parent build/parent_1.so build/parent_2.so \
         --new duckdb-adaptive-compression_amd/libadacodec.so --out launch_cost.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "duckdb-adaptive-compression_amd")
ROWS, NGROUPS = 1024, 6


def binding(name, lib_path):
    """the package once more under another module name, on another library"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG_DIR, "__init__.py"),
                                                  submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(lib_path)  # before the first lib() call
    return mod


class Calls:
    """the timed entry points on one library: name -> (call, its output buffer, words to compare)"""

    def __init__(self, adac):
        self.ctx = ctx = adac.Context(0)
        rng = np.random.default_rng(14)
        counts = np.array([ROWS], dtype=np.uint32)
        self.keep = []

        def col(lo, hi, dtype, v=None):
            v = rng.integers(lo, hi, size=ROWS).astype(dtype) if v is None else v
            lay = adac.Layout(ctx, dtype, counts)
            d_words = ctx.alloc(lay.max_arena_words * 8 + 128).zero()
            d_vals = ctx.upload(v)
            lay.encode(d_vals, d_words)
            ctx.sync()
            self.keep.append((lay, d_words))
            return lay, d_words, v

        (a, wa, _), (b, wb, _), (c, wc, _) = col(900, 105000, np.int32), col(0, 11, np.uint8), col(-3, 9, np.int16)
        (q, wq, qv), (k, wk, _), (d, wd, _) = col(1, 51, np.uint32), col(0, NGROUPS, np.uint8), col(0, 105000, np.int32)
        mask = ctx.upload(rng.integers(0, 2 ** 63, size=ROWS // 64 + 1, dtype=np.uint64))
        member_set = ctx.upload(rng.integers(0, 2 ** 63, size=2, dtype=np.uint64))
        out_q1, out_p3 = ctx.alloc(8 * 7 * (NGROUPS + 1)), ctx.alloc(8 * (NGROUPS + 1))
        bm, cnt = ctx.alloc(8 * (ROWS // 64 + 1)), ctx.alloc(8)
        v = rng.integers(0, 4000, size=ROWS).astype(np.int32)
        d_vals = ctx.upload(v)
        plan = adac.BitpackingPlan(ctx, v.dtype, d_vals, ROWS)
        d_blocks = ctx.alloc(plan.nseg * plan.BLOCK_STRIDE + 64)
        plan.write(d_vals, d_blocks)
        ctx.sync()
        bp_counts = np.array([plan.segment(i)[1] for i in range(plan.nseg)], dtype=np.uint32)
        bp = adac.BitpackingLayout(ctx, v.dtype, np.arange(plan.nseg, dtype=np.uint64) * plan.BLOCK_STRIDE, bp_counts)
        # the dense-key scans: q is the key, [1, 50] its domain of 56 map bytes; a key's code is a function of the key,
        # so that the build stores the same byte whichever row comes last
        code, wcode, _ = col(0, 0, np.uint8, (qv % NGROUPS).astype(np.uint8))
        d_map = ctx.upload(rng.integers(0, NGROUPS + 1, size=56).astype(np.uint8))
        built, seg = ctx.alloc(56), ctx.alloc(8)
        dn_s, dn_c = ctx.alloc(8 * 50), ctx.alloc(8 * 50)
        mp_s, mp_c, pm_ab, pm_a, pm_c = (ctx.alloc(8 * (NGROUPS + 1)) for _ in range(5))
        # the cheapest entry points, without a mask: what a change to the host side of every call shows on first
        sums, range_out, bp_sums = ctx.alloc(8), ctx.alloc(4 * ROWS + 16), ctx.alloc(8 * plan.nseg)
        self.keep += [mask, member_set, d_blocks, bp, plan, d_map]
        self.calls = {
            "adac_scan_sum": (lambda: a.scan_sum(wa, sums), sums, 1),
            "adac_scan_count_between": (lambda: a.scan_count_between(wa, 5000, 60000, cnt), cnt, 1),
            "adac_unpack_range": (lambda: a.unpack_range(wa, 0, 0, ROWS, range_out), range_out, ROWS // 2),
            "adac_bp_scan_sum": (lambda: bp.scan_sum(d_blocks, bp_sums), bp_sums, plan.nseg),
            "adac_scan_group_sum_q1": (lambda: a.scan_group_sum_q1(wa, b, wb, c, wc, q, wq, k, wk, NGROUPS, out_q1, mask),
                                       out_q1, 7 * (NGROUPS + 1)),
            "adac_scan_group_sum_product3": (lambda: a.scan_group_sum_product3(wa, b, wb, c, wc, k, wk, NGROUPS, out_p3,
                                                                              None, mask), out_p3, NGROUPS + 1),
            "adac_scan_select_compare": (lambda: a.scan_select_compare(wa, d, wd, adac.CMP_LT, bm, cnt, mask),
                                         bm, ROWS // 64),
            "adac_scan_select_member": (lambda: b.scan_select_member(wb, member_set, 0, 11, bm, cnt, mask), bm, ROWS // 64),
            "adac_bp_scan_select_between": (lambda: bp.scan_select_between(d_blocks, 100, 2000, bm, cnt, mask),
                                            bm, ROWS // 64),
            "adac_scan_group_sum_dense": (lambda: q.scan_group_sum_dense(wq, a, wa, 1, 50, dn_s, dn_c, seg, mask), dn_s, 50),
            "adac_scan_group_sum_mapped": (lambda: q.scan_group_sum_mapped(wq, a, wa, d_map, 1, 50, NGROUPS, mp_s, mp_c,
                                                                          seg, mask), mp_s, NGROUPS + 1),
            "adac_scan_group_sum_product_mapped": (lambda: q.scan_group_sum_product_mapped(
                wq, a, wa, b, wb, d_map, 1, 50, NGROUPS, pm_ab, pm_a, pm_c, seg, mask), pm_ab, NGROUPS + 1),
            "adac_scan_build_map": (lambda: q.scan_build_map(wq, code, wcode, 1, 50, built, 255, seg, mask), built, 7),
        }

    def time(self, name, calls):
        fn = self.calls[name][0]
        fn()
        self.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        self.ctx.sync()
        return (time.perf_counter() - t0) / calls * 1e6

    def time_enqueue(self, name, burst, reps):
        fn = self.calls[name][0]
        spent = 0.0
        for _ in range(reps):
            self.ctx.sync()
            t0 = time.perf_counter()
            for _ in range(burst):
                fn()
            spent += time.perf_counter() - t0
        self.ctx.sync()
        return spent / (burst * reps) * 1e6

    def result(self, name):
        fn, buf, words = self.calls[name]
        fn()
        self.ctx.sync()
        return buf.download(np.uint64, words).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs=2, required=True, help="the parent's build under two file names")
    ap.add_argument("--new", required=True)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--burst", type=int, default=32)
    ap.add_argument("--only", nargs="+", default=None, help="time these entry points only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = {"parent_1": a.parent[0], "parent_2": a.parent[1], "new": a.new}
    sets = {tag: Calls(binding("adac_" + tag, path)) for tag, path in libs.items()}
    unknown = sorted(set(a.only or ()) - set(sets["new"].calls))
    if unknown:
        ap.error("--only: not a timed entry point: %s (known: %s)" % (", ".join(unknown), ", ".join(sets["new"].calls)))
    names = [n for n in sets["new"].calls if a.only is None or n in a.only]
    first = {n: sets["parent_1"].result(n) for n in names}
    for tag, s in sets.items():
        for n in names:
            assert s.result(n) == first[n], (tag, n)
    us = {n: {tag: [] for tag in libs} for n in names}
    host = {n: {tag: [] for tag in libs} for n in names}
    tags = list(libs)
    for r in range(a.rounds):
        order = tags[r % 3:] + tags[:r % 3]  # every library takes every place in the round
        for n in names:
            for tag in order:
                us[n][tag].append(sets[tag].time(n, a.calls))
            for tag in order:
                host[n][tag].append(sets[tag].time_enqueue(n, a.burst, a.calls // a.burst // 4))

    def cell(v):
        med = {tag: statistics.median(x) for tag, x in v.items()}
        parent = statistics.median(v["parent_1"] + v["parent_2"])
        margin = abs(med["parent_1"] - med["parent_2"])
        return {"median_us": {t: round(x, 3) for t, x in med.items()},
                "min_us": {t: round(min(x), 3) for t, x in v.items()},
                "parent_median_us": round(parent, 3), "margin_us": round(margin, 3),
                "new_minus_parent_us": round(med["new"] - parent, 3),
                "within_margin": bool(med["new"] <= parent + margin),
                "rounds_us": {t: [round(y, 3) for y in x] for t, x in v.items()}}

    cells = {n: dict(cell(us[n]), host_only=cell(host[n])) for n in names}
    table = {"unit": "microseconds of wall time per call: %d back-to-back calls + one sync, median of %d rounds, "
                     "libraries alternating in one process; one segment of %d rows, a mask wherever the call takes "
                     "one (not adac_scan_sum, _scan_count_between, _unpack_range, _bp_scan_sum); "
                     "outputs equal between the libraries.  host_only: the same per call over bursts of %d calls "
                     "enqueued on an idle stream, the sync not timed" % (a.calls, a.rounds, ROWS, a.burst),
             "libs": libs, "cells": cells}
    txt = json.dumps(table, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)
    keys = ("median_us", "min_us", "margin_us", "new_minus_parent_us", "within_margin")
    print(json.dumps({n: {"back_to_back": {k: c[k] for k in keys}, "host_only": {k: c["host_only"][k] for k in keys}}
                      for n, c in cells.items()}, indent=1))


if __name__ == "__main__":
    main()
