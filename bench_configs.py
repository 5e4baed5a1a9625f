#!/usr/bin/env python3
"""Secondary harness (NOT the driver's bench.py): the reference's other workloads through the drop-in path,
one JSON object on stdout.  Numbers go to profiles/ and DESIGN.md.

  plugin_scan  benchmark/micro/succinct/sequential.cpp (SELECT * full scans): a column loaded and scanned through
               the C++ host mirror in ColumnData::ScanVector's call pattern (2048-row Scan calls that return
               rows to HOST memory), with and without the decoded-segment cache — the PCIe-inclusive path.
  adaptive     zipf_over_time.cpp / zipf_distribution_diff_skews.cpp: segment-access traces with Zipf skew
               0.5 / 1.0 / 2.0, one policy round per period: resident bytes, flips and re-encode rate.
"""
import importlib
import json
import os
import sys
import time
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "duckdb-adaptive-compression_amd"
# host mirrors of the kernels' rule "which form takes this scan group": they live in the package (forms.py) and stay
# importable from here under the names they had when they were defined in this file
forms = importlib.import_module(PKG + ".forms")
product_form_groups, group_product_form_groups = forms.product_form_groups, forms.group_product_form_groups
group_product3_form_groups, group_q1_form_groups = forms.group_product3_form_groups, forms.group_q1_form_groups


def load(db, lay, dtype, values):
    dtype = np.dtype(dtype)
    row = 0
    for count, cap in lay.appender_segments(len(values), dtype.itemsize):
        s = db.create_segment(dtype, start=row, segment_size=cap * dtype.itemsize)
        v = values[row:row + count]
        for off in range(0, count, 2048):
            s.append(v, offset=off, count=min(2048, count - off))
        row += count


PCIE_GBS = 63.0  # PCIe Gen5 x16, one direction (spec)


def plugin_scan(host, lay, n=int(os.environ.get("PLUGIN_SCAN_ROWS", 200_000_000))):
    values = np.arange(n, dtype=np.uint32)  # SuccinctSequentialInsert / C1 column
    out = {"rows": n, "dtype": "u32", "vector_size": 2048, "pcie_spec_GBps": PCIE_GBS, "variants": {}}
    ncpu = len(os.sched_getaffinity(0))
    variants = [("per_vector_device_decode", dict(decoded_cache_bytes=0), (1,), min(n, 4_000_000)),
                ("decoded_segment_cache", dict(decoded_cache_bytes=192 << 20, scan_lanes=8, prefetch_segments=8),
                 (1, 2, 4, 8, 16), n),
                ("decoded_segment_cache_2_pools_on_one_gpu",
                 dict(device=[0, 0], decoded_cache_bytes=96 << 20, scan_lanes=4, prefetch_segments=8), (1, 8), n)]
    for name, kw, thread_counts, rows_here in variants:
        kw = dict(kw)
        device = kw.pop("device", 0)
        db = host.Database(device, arena_bytes=1 << 30, **kw)
        t0 = time.perf_counter()
        load(db, lay, np.uint32, values[:rows_here])
        db.compact_all()
        t_load = time.perf_counter() - t0
        rec = {"rows": rows_here, "load_and_compact_s": t_load, "total_data_size": db.total_data_size, "scans": {}}
        for th in thread_counts:
            if th > ncpu:
                continue
            # cold: the cache (192 MiB) is smaller than the column (800 MB) and LRU, so every pass decodes and copies
            # every segment again; warm is measured on a prefix that fits
            cs, sec_cold, rows = db.full_scan(threads=th)
            assert cs == rows_here * (rows_here - 1) // 2
            cs, sec_cold2, rows = db.full_scan(threads=th)
            sec = min(sec_cold, sec_cold2)
            rec["scans"]["threads_%d" % th] = {
                "cold_scan_rows_per_s": rows / sec, "d2h_GBps": rows * 4 / sec / 1e9,
                "fraction_of_pcie_spec": rows * 4 / sec / 1e9 / PCIE_GBS}
        if kw.get("decoded_cache_bytes"):
            fit = [s for s in db.segments][:400]   # ~100 MB: stays resident
            db.full_scan(fit)
            for th in (1, 8):
                cs, sec_warm, rows = db.full_scan(fit, threads=th)
                rec["scans"]["warm_threads_%d" % th] = {"rows_per_s": rows / sec_warm}
        rec["cache"] = db.cache_stats()
        rec["prefetch"] = db.prefetch_stats()
        out["variants"][name] = rec
        db.close()
    return out


def adaptive(host, wl, nseg=400, rows=32767, periods=4):
    rng = np.random.default_rng(3)
    out = {"segments": nseg, "rows_per_segment": rows, "skews": {}}
    data = [((i << 34) + rng.integers(0, 1 << (10 + i % 12), size=rows)).astype(np.uint64) for i in range(nseg)]
    for skew, cache in ((0.5, 0), (1.0, 0), (2.0, 0), (0.5, 128 << 20)):
        # the last variant keeps decoded images of the packed segments it touches in the page-locked cache: a
        # look-up into a packed segment is then a memcpy, not a device round trip
        db = host.Database(0, adaptive=True, arena_bytes=512 << 20, decoded_cache_bytes=cache, prefetch_segments=1)
        db.reserve_staging(nseg * rows * 8 + (1 << 20))   # one-time page-locking kept out of the first policy round
        for i in range(nseg):
            s = db.create_segment(np.uint64, start=i * rows)
            for off in range(0, rows, 2048):
                s.append(data[i], offset=off, count=min(2048, rows - off))
        rec = {"raw_bytes": db.total_data_size, "periods": []}
        for p in range(periods):
            trace = wl.zipf_column(20000, np.uint32, domain=nseg, skew=skew, seed=500 + p, threads=1) - 1
            t0 = time.perf_counter()
            scanned = 0
            for i in trace:
                db.segments[int(i)].scan(0, 2048)
                scanned += 2048
            t_scan = time.perf_counter() - t0
            before = [s.compacted for s in db.segments]
            t0 = time.perf_counter()
            db.policy_step(0.90)
            t_policy = time.perf_counter() - t0
            after = [s.compacted for s in db.segments]
            packed = sum(1 for a, b in zip(before, after) if b and not a)
            expanded = sum(1 for a, b in zip(before, after) if a and not b)
            rec["periods"].append({
                "lookups_per_s": len(trace) / t_scan, "scanned_rows_per_s": scanned / t_scan,
                "resident_bytes": db.total_data_size, "arena_bytes": db.arena_used_bytes,
                "policy_step_s": t_policy, "segments_packed": packed, "segments_expanded": expanded,
                "reencode_raw_GBps": (packed + expanded) * rows * 8 / t_policy / 1e9 if t_policy > 0 else None,
            })
        out["skews"][str(skew) + ("_decoded_cache" if cache else "")] = rec
        db.close()
    return out



# ----------------------------------------------------------------------------------------------------------------------
# what the scan jobs below share: the synthetic lineitem table, the column encoders, the timers, Q6's and Q1's plans
# ----------------------------------------------------------------------------------------------------------------------
INT32_MIN_BITS = 0x80000000  # int32's minimum as the uint32 bit pattern the scans take for "no lower bound"

# TPC-H lineitem at SF10 size, synthetic: int32 columns in integer decimals and the engine's dictionary code of
# (l_returnflag, l_linestatus) as a 6-valued uint8
LINEITEM = {
    "code": lambda rng, n: rng.choice(6, size=n, p=[.2466, .2534, .0004, .2500, .2490, .0006]).astype(np.uint8),
    "l_quantity": lambda rng, n: rng.integers(1, 51, size=n).astype(np.int32),
    "l_extendedprice": lambda rng, n: rng.integers(90_000, 10_495_000, size=n).astype(np.int32),   # cents
    "l_partkey": lambda rng, n: rng.integers(1, 2_000_001, size=n).astype(np.int32),
    "l_shipdate": lambda rng, n: rng.integers(8036, 10562, size=n).astype(np.int32),   # days since 1970: 1992-01-02 .. 1998-12-01
    # independent uniform draws in l_shipdate's range: dbgen's commit and receipt dates follow the ship date closely, so
    # a predicate between two of these selects more rows here than on the real table
    "l_commitdate": lambda rng, n: rng.integers(8036, 10562, size=n).astype(np.int32),
    "l_receiptdate": lambda rng, n: rng.integers(8036, 10562, size=n).astype(np.int32),
    "l_discount": lambda rng, n: rng.integers(0, 11, size=n).astype(np.int32),          # percent
    "l_tax": lambda rng, n: rng.integers(0, 9, size=n).astype(np.int32),                # percent
}
Q1_CUTOFF_DAY = 10511  # l_shipdate <= cutoff keeps about 98 % of the uniform dates, as Q1's WHERE clause does


def lineitem(rng, n, names):
    """The named columns, drawn from rng in the order given (a job's seed and draw order are part of its numbers)."""
    return {name: LINEITEM[name](rng, n) for name in names}


def packed_bytes(descs):
    return int(((descs["count"].astype(np.uint64) * descs["width"] + 63) // 64 * 8).sum())


# a column on the device; `lay` and the device image come first in both, which is all q6_selects looks at
Encoded = namedtuple("Encoded", "lay words nbytes widths descs")        # packed by adac_encode
Blocks = namedtuple("Blocks", "lay words nseg nbytes counts info")      # DuckDB BITPACKING blocks, one per stride


def encode_column(adac, ctx, v, counts):
    lay = adac.Layout(ctx, v.dtype, counts)
    d_vals = ctx.upload(v)
    d_words = ctx.alloc(lay.max_arena_words * 8 + 16).zero()
    lay.encode(d_vals, d_words)
    ctx.sync()
    d_vals.free()
    descs = lay.get_descs()
    return Encoded(lay, d_words, packed_bytes(descs), sorted(set(descs["width"].tolist())), descs)


def bitpacking_blocks(adac, ctx, comp, dtype, stride=262144):
    """The block image of an oracle.bitpacking.Compressed column on the device, one block per `stride` bytes."""
    from oracle import bitpacking as bp
    nseg = comp.nseg
    buf = np.zeros(nseg * stride + 64, dtype=np.uint8)
    counts = np.zeros(nseg, dtype=np.uint32)
    used = 0
    for i in range(nseg):
        buf[i * stride:i * stride + bp.BLOCK_SIZE] = comp.block(i)
        counts[i] = comp.count(i)
        used += comp.size(i)
    d_blocks = ctx.upload(buf)
    lay = adac.BitpackingLayout(ctx, dtype, np.arange(nseg, dtype=np.uint64) * stride, counts)
    info = {"segments": nseg, "groups": int(lay.ngroups), "modes": comp.groups_by_mode(),
            "width_of_group_0": comp.group_info(0, 0)[2]}
    return Blocks(lay, d_blocks, nseg, used, counts, info)


def timed(ctx, fn, reps=20, warm=True):
    """ms per call of `reps` back-to-back calls between two events, after one untimed call"""
    if warm:
        fn()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


ROUNDS, INNER = 8, 5


def timed_interleaved(ctx, entries, rounds=ROUNDS, inner=INNER):
    """{name: ms per call in each round}.  Warm and interleaved: an untimed round, then `rounds` rounds in which every
    entry runs `inner` times back to back between two events of its own (one call alone, 0.1 ms, would be timed together
    with its launch gap).  With every entry following a different one, none starts on a cache it warmed alone."""
    samples = {name: [] for name, _ in entries}
    for r in range(rounds + 1):
        for name, fn in entries:
            ctx.timer_start()
            for _ in range(inner):
                fn()
            t = ctx.timer_stop() / inner
            if r:
                samples[name].append(t)
    return samples


Q6_DATES, Q6_DISCOUNT, Q6_MAX_QUANTITY = (8766, 9130), (5, 7), 23   # 1994-01-01 .. 1994-12-31, percent, l_quantity < 24


def q6_selects(cols, bm, d_cnt):
    """Q6's WHERE clause as three chained selection scans; the final bitmap is bm[2].  cols: Encoded or Blocks by name."""
    def select(name, *args):
        lay, image = cols[name][:2]
        lay.scan_select_between(image, *args)

    select("l_shipdate", *Q6_DATES, bm[0], d_cnt)
    select("l_discount", *Q6_DISCOUNT, bm[1], d_cnt, bm[0])
    select("l_quantity", INT32_MIN_BITS, Q6_MAX_QUANTITY, bm[2], d_cnt, bm[1])


def q6_mask(cols):
    return ((cols["l_shipdate"] >= Q6_DATES[0]) & (cols["l_shipdate"] <= Q6_DATES[1]) &
            (cols["l_discount"] >= Q6_DISCOUNT[0]) & (cols["l_discount"] <= Q6_DISCOUNT[1]) &
            (cols["l_quantity"] <= Q6_MAX_QUANTITY))


def q1_outputs(s, c):
    """Q1's eight output columns per group, as integers, from the sums s["q" "p" "d" "pd" "pt" "pdt"] and the counts
    c["q" "p" "d"] (ngroups + 1 = 7 entries each).  In integer decimals
      sum_disc_price = 100 SUM(p) - SUM(p d)
      sum_charge     = 10000 SUM(p) + 100 SUM(p t) - 100 SUM(p d) - SUM(p d t)
    and the three averages are exact (sum, count) pairs."""
    assert all(v[6] == 0 for v in list(s.values()) + list(c.values())), "no row has a key >= 6"
    g6 = range(6)
    return {"sum_qty": [s["q"][g] for g in g6],
            "sum_base_price": [s["p"][g] for g in g6],
            "sum_disc_price": [100 * s["p"][g] - s["pd"][g] for g in g6],
            "sum_charge": [10000 * s["p"][g] + 100 * s["pt"][g] - 100 * s["pd"][g] - s["pdt"][g] for g in g6],
            "avg_qty": [(s["q"][g], c["q"][g]) for g in g6],
            "avg_price": [(s["p"][g], c["p"][g]) for g in g6],
            "avg_disc": [(s["d"][g], c["d"][g]) for g in g6],
            "count_order": [c["p"][g] for g in g6]}


def q1_expected(cols, bins):
    """numpy's Q1 over the rows of each bin (one boolean mask per group), in q1_outputs' form"""
    q64, p64, d64, t64 = (cols[k].astype(np.int64) for k in ("l_quantity", "l_extendedprice", "l_discount", "l_tax"))
    rows = [int(b.sum()) for b in bins]
    sq, sp, sd = ([int(v[b].sum()) for b in bins] for v in (q64, p64, d64))
    return {"sum_qty": sq, "sum_base_price": sp,
            "sum_disc_price": [int((p64[b] * (100 - d64[b])).sum()) for b in bins],
            "sum_charge": [int((p64[b] * (100 - d64[b]) * (100 + t64[b])).sum()) for b in bins],
            "avg_qty": list(zip(sq, rows)), "avg_price": list(zip(sp, rows)), "avg_disc": list(zip(sd, rows)),
            "count_order": rows}


def q1_json(outputs):
    return {k: [list(x) if isinstance(x, tuple) else x for x in v] for k, v in outputs.items()}


def q1_setup(adac, ctx, n):
    """What q1_full_packed and q1_fused_packed share: the six columns (seed 1995) encoded on one segment layout, the
    l_shipdate select and the six grouped calls under its bitmap, every result in a (sums, counts) pair of its own."""
    t = SimpleNamespace()
    t.cols = lineitem(np.random.default_rng(1995), n,
                      ("code", "l_extendedprice", "l_shipdate", "l_quantity", "l_discount", "l_tax"))
    counts = adac.appender_segment_counts(n, 4)
    t.enc = enc = {k: encode_column(adac, ctx, t.cols[k], counts)
                   for k in ("code", "l_shipdate", "l_quantity", "l_extendedprice", "l_discount", "l_tax")}
    (klay, kwords), (dlay, dwords), (qlay, qwords), (play, pwords), (clay, cwords), (tlay, twords) = (
        e[:2] for e in enc.values())
    t.d_filter = d_filter = ctx.alloc((n + 63) // 64 * 8 + 8)
    d_selcnt = ctx.alloc(len(counts) * 8)
    t.res = res = {k: (ctx.alloc(7 * 8), ctx.alloc(7 * 8)) for k in ("q", "p", "d", "pd", "pt", "pdt")}
    t.select = lambda: dlay.scan_select_between(dwords, INT32_MIN_BITS, Q1_CUTOFF_DAY, d_filter, d_selcnt)

    def sum_pdt(mask=True, with_counts=False):
        play.scan_group_sum_product3(pwords, clay, cwords, tlay, twords, klay, kwords, 6, res["pdt"][0],
                                     res["pdt"][1] if with_counts else None, d_filter if mask else None)

    t.sum_pdt = sum_pdt
    t.six = (
        ("group_sum_quantity_masked", lambda: qlay.scan_group_sum_valid(qwords, klay, kwords, d_filter, 6, *res["q"])),
        ("group_sum_price_masked", lambda: play.scan_group_sum_valid(pwords, klay, kwords, d_filter, 6, *res["p"])),
        ("group_sum_discount_masked", lambda: clay.scan_group_sum_valid(cwords, klay, kwords, d_filter, 6, *res["d"])),
        ("group_sum_product_price_disc_masked",
         lambda: play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, res["pd"][0], None, d_filter)),
        ("group_sum_product_price_tax_masked",
         lambda: play.scan_group_sum_product(pwords, tlay, twords, klay, kwords, 6, res["pt"][0], None, d_filter)),
        ("group_sum_product3_masked", sum_pdt))
    t.keep = t.cols["l_shipdate"] <= Q1_CUTOFF_DAY
    t.all_bins = [t.cols["code"] == g for g in range(6)]
    t.kept_bins = [b & t.keep for b in t.all_bins]
    return t


def bitpacking_columns(n):
    rng = np.random.default_rng(11)
    return {
        "for_u32_w20": (5_000_000 + rng.integers(0, 1 << 20, size=n)).astype(np.uint32),
        "delta_for_i64_sorted": (10 ** 12 + np.cumsum(rng.integers(0, 1 << 9, size=n))).astype(np.int64),
        "for_u64_w32": (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) + np.uint64(1 << 40)).astype(np.uint64),
    }


def bitpacking_fused_scans(adac, n=50_000_000):
    """Fused scans on BITPACKING blocks (adac_bp_scan_*) beside the decode of the same blocks, same process: per-call
    HIP-event times of scan_sum, scan_select_between at about 10 % selectivity and adac_bp_unpack over
    bitpacking_scan's three columns, after the results were checked against numpy."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    out = {"rows": n, "cases": []}
    for name, v in bitpacking_columns(n).items():
        comp = bp.Compressed(v)
        lay, d_blocks, nseg, used, counts, info = bitpacking_blocks(adac, ctx, comp, v.dtype)
        d_out = ctx.alloc(n * v.dtype.itemsize + 64)
        d_sum, d_cnt, d_bm = ctx.alloc(nseg * 8), ctx.alloc(nseg * 8), ctx.alloc((n + 63) // 64 * 8 + 8)
        lo, hi = (int(x) for x in np.quantile(v, [0.45, 0.55]))
        lay.unpack(d_blocks, d_out)
        lay.scan_sum(d_blocks, d_sum)
        lay.scan_select_between(d_blocks, lo, hi, d_bm, d_cnt)
        ctx.sync()
        assert np.array_equal(d_out.download(v.dtype, n), v)
        bounds = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        wide = v.astype(np.int64 if v.dtype.kind == "i" else np.uint64).view(np.uint64)
        want = np.add.reduceat(wide, bounds[:-1])
        assert np.array_equal(d_sum.download(np.uint64, nseg), want), "SUM parity"
        hit = (v >= lo) & (v <= hi)
        assert np.array_equal(d_cnt.download(np.uint64, nseg), np.add.reduceat(hit.astype(np.uint64), bounds[:-1]))
        words = np.packbits(np.concatenate([hit, np.zeros((-n) % 64, dtype=bool)]), bitorder="little").view(np.uint64)
        assert np.array_equal(d_bm.download(np.uint64, len(words)), words), "bitmap parity"
        ms = {}
        for what, fn in (("decode", lambda: lay.unpack(d_blocks, d_out)), ("scan_sum", lambda: lay.scan_sum(d_blocks, d_sum)),
                         ("select", lambda: lay.scan_select_between(d_blocks, lo, hi, d_bm, d_cnt)),
                         ("decode_again", lambda: lay.unpack(d_blocks, d_out)),
                         ("scan_sum_again", lambda: lay.scan_sum(d_blocks, d_sum))):
            ms[what] = timed(ctx, fn)
        dec, ssum = min(ms["decode"], ms["decode_again"]), min(ms["scan_sum"], ms["scan_sum_again"])
        out["cases"].append({
            "name": name, "dtype": str(v.dtype), "segments": nseg, "groups": info["groups"], "compressed_bytes": used,
            "modes": info["modes"], "selectivity": float(hit.mean()), "ms": ms,
            "decode_ms": dec, "scan_sum_ms": ssum, "select_ms": ms["select"],
            "scan_sum_over_decode": ssum / dec, "select_over_decode": ms["select"] / dec,
            "scan_sum_block_TBps": used / (ssum * 1e-3) / 1e12, "select_block_TBps": used / (ms["select"] * 1e-3) / 1e12,
            "decode_block_TBps": used / (dec * 1e-3) / 1e12,
        })
        del lay, d_blocks, d_out, d_sum, d_cnt, d_bm, comp
    ctx.close()
    return out


def bitpacking_scan(adac, n=50_000_000):
    """Full scan of on-disk BITPACKING segments: blocks written by the oracle's restatement of the
    reference's compress (CPU, untimed), decoded on the device; rates from HIP events on the codec stream."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    out = {"rows": n, "cases": []}
    stride = 262144
    for name, v in bitpacking_columns(n).items():
        t0 = time.perf_counter()
        comp = bp.Compressed(v)
        t_cpu = time.perf_counter() - t0
        lay, d_blocks, nseg, used, _, info = bitpacking_blocks(adac, ctx, comp, v.dtype, stride)
        d_out = ctx.alloc(n * v.dtype.itemsize + 64)
        lay.unpack(d_blocks, d_out)
        ctx.sync()
        assert np.array_equal(d_out.download(v.dtype, n), v)
        ms = timed(ctx, lambda: lay.unpack(d_blocks, d_out), warm=False)
        # GPU compress of the same column: statistics + host decisions + group writes (wall time, host included)
        d_vals = ctx.upload(v)
        t0 = time.perf_counter()
        plan = adac.BitpackingPlan(ctx, v.dtype, d_vals, n)
        d_new = ctx.alloc(plan.nseg * plan.BLOCK_STRIDE + 64)
        plan.write(d_vals, d_new)
        ctx.sync()
        t_gpu_compress = time.perf_counter() - t0
        assert plan.nseg == nseg and plan.groups_by_mode() == info["modes"]
        img = d_new.download(np.uint8, nseg * plan.BLOCK_STRIDE)
        assert all(np.array_equal(img[i * stride:i * stride + comp.size(i)], comp.block(i)[:comp.size(i)])
                   for i in range(0, nseg, max(1, nseg // 16)))
        del d_new, d_vals, plan
        out["cases"].append({
            "gpu_compress_values_per_s": n / t_gpu_compress, "gpu_compress_s": t_gpu_compress,
            "name": name, "dtype": str(v.dtype), "segments": nseg, "compressed_bytes": used,
            "modes": info["modes"], "cpu_compress_values_per_s": n / t_cpu, "decode_ms": ms,
            "decode_values_per_s": n / (ms * 1e-3),
            "algorithmic_GBps": (used + n * v.dtype.itemsize) / (ms * 1e-3) / 1e9,
        })
        del lay, d_blocks, d_out, comp
    ctx.close()
    return out


def q6_packed(adac, n=59_986_052):
    """C3's Q6 shape on packed columns: WHERE l_shipdate in a year AND l_discount BETWEEN
    5 AND 7 AND l_quantity < 24 -> SUM(l_extendedprice), on four int32 columns of TPC-H SF10 size that share
    their segment layout.  Three filter scans chain their selection bitmaps, the fourth scan aggregates under the
    final bitmap; nothing is decoded to HBM.  (Q6 proper sums price * discount: that is q6_product_packed below, on
    adac_scan_sum_product.)  Beside it: the materialising plan (decode the four columns, then filter)
    counted at its decode cost alone."""
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1994), n, ("l_shipdate", "l_discount", "l_quantity", "l_extendedprice"))
    counts = adac.appender_segment_counts(n, 4)
    enc = {name: encode_column(adac, ctx, v, counts) for name, v in cols.items()}
    total_bytes = sum(e.nbytes for e in enc.values())
    nw = (n + 63) // 64
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_cnt = ctx.alloc(len(counts) * 8)
    d_sum = ctx.alloc(len(counts) * 8)
    ship, disc, price = enc["l_shipdate"], enc["l_discount"], enc["l_extendedprice"]

    def q6():
        q6_selects(enc, bm, d_cnt)
        price.lay.scan_sum(price.words, d_sum, bm[2])

    q6()
    ctx.sync()
    m = q6_mask(cols)
    got = int(d_sum.download(np.uint64, len(counts)).sum(dtype=np.uint64))
    assert got == int(cols["l_extendedprice"][m].astype(np.int64).sum()), "Q6 parity"
    assert int(d_cnt.download(np.uint64, len(counts)).sum()) == int(m.sum())
    by_group = {}
    for group in (2, 4, 8, 16):
        adac.set_tuning("scan_tiles_per_wg", group)
        by_group[group] = timed(ctx, q6)
    adac.set_tuning("scan_tiles_per_wg", 0)
    ms = timed(ctx, q6)
    steps = {}
    for name, fn in (("select_shipdate", lambda: ship.lay.scan_select_between(ship.words, *Q6_DATES, bm[0], d_cnt)),
                     ("select_discount_masked", lambda: disc.lay.scan_select_between(disc.words, *Q6_DISCOUNT, bm[1], d_cnt, bm[0])),
                     ("sum_price_masked", lambda: price.lay.scan_sum(price.words, d_sum, bm[2])),
                     ("count_shipdate", lambda: ship.lay.scan_count_between(ship.words, *Q6_DATES, d_cnt))):
        steps[name] = timed(ctx, fn)
    # filter then project: only the surviving rows of l_extendedprice are decoded
    d_sel = ctx.alloc(int(m.sum()) * 4 + 64)
    got = price.lay.unpack_selected(price.words, bm[2], d_sel)
    assert got == int(m.sum()) and np.array_equal(d_sel.download(np.int32, got), cols["l_extendedprice"][m])
    steps["project_price_selected"] = timed(ctx, lambda: price.lay.unpack_selected(price.words, bm[2], d_sel, None, False),
                                            warm=False)
    d_out = ctx.alloc(n * 4 + 64)

    def decode_four():
        for e in enc.values():
            e.lay.unpack(e.words, d_out)

    ms_dec = timed(ctx, decode_four, warm=False)
    out = {"rows": n, "selected_rows": int(m.sum()), "widths": {k: e.widths for k, e in enc.items()},
           "packed_bytes": total_bytes, "q6_on_packed_ms": ms, "q6_rows_per_s": n / (ms * 1e-3),
           "q6_packed_read_GBps": total_bytes / (ms * 1e-3) / 1e9,
           "decode_four_columns_ms": ms_dec,
           "decode_four_columns_total_GBps": (total_bytes + 4 * n * 4) / (ms_dec * 1e-3) / 1e9, "q6_ms_by_scan_tiles_per_wg": by_group, "step_ms": steps,
           "note": "q6_on_packed = 3 chained filter scans (selection bitmaps) + 1 masked SUM; decode_four_columns is "
                   "only the materialisation a decode-then-filter plan would pay before filtering"}
    ctx.close()
    return out


def q1_packed(adac, n=59_986_052):
    """C3's Q1 shape on packed columns ("Q1 = group-by sum"; benchmark log TPCH_runtime.txt:2-6):
    SUM(l_quantity), SUM(l_extendedprice), SUM(l_partkey), COUNT(*) GROUP BY (l_returnflag, l_linestatus) on int32
    columns of TPC-H SF10 size that share their segment layout; the group code is a 6-valued uint8 column (the
    engine's dictionary code of the two flags).  One adac_scan_group_sum per aggregated column, nothing decoded to
    HBM; checked against numpy's GROUP BY.  Beside it: decoding the same columns (what the reference's engine needs
    before its hash aggregate can start)."""
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1992), n, ("code", "l_quantity", "l_extendedprice", "l_partkey"))
    code = cols.pop("code")
    counts = adac.appender_segment_counts(n, 4)
    klay, kwords, kbytes, kwidths, _ = encode_column(adac, ctx, code, counts)
    d_sums = ctx.alloc(7 * 8)
    d_cnts = ctx.alloc(7 * 8)
    out = {"rows": n, "groups": 6, "key_widths": kwidths, "key_packed_bytes": kbytes, "columns": []}
    total_ms, total_bytes = 0.0, 0
    for name, v in cols.items():
        lay, words, nbytes, widths, _ = encode_column(adac, ctx, v, counts)
        group_sum = lambda: lay.scan_group_sum(words, klay, kwords, 6, d_sums, d_cnts)
        group_sum()
        ctx.sync()
        got_s = d_sums.download(np.uint64, 7).tolist()
        got_c = d_cnts.download(np.uint64, 7).tolist()
        for g in range(6):
            m = code == g
            assert got_c[g] == int(m.sum()) and got_s[g] == int(v[m].astype(np.int64).sum()), "Q1 parity"
        assert got_c[6] == 0
        ms = timed(ctx, group_sum, warm=False)
        # the same aggregate through the staged-LDS kernel alone (round 2's form), for the record
        adac.set_tuning("group_sum_rw", 0)
        ms_lds = timed(ctx, group_sum)
        assert d_sums.download(np.uint64, 7).tolist() == got_s and d_cnts.download(np.uint64, 7).tolist() == got_c
        adac.set_tuning("group_sum_rw", 1)
        d_out = ctx.alloc(n * 4 + 64)
        ms_dec = timed(ctx, lambda: lay.unpack(words, d_out))
        del d_out
        total_ms += ms
        total_bytes += nbytes + kbytes
        out["columns"].append({"column": name, "widths": widths, "packed_bytes": nbytes, "group_sum_ms": ms,
                               "rows_per_s": n / (ms * 1e-3), "packed_read_GBps": (nbytes + kbytes) / (ms * 1e-3) / 1e9,
                               "staged_lds_kernel_ms": ms_lds, "decode_only_ms": ms_dec})
        del lay, words
    out["q1_three_aggregates_ms"] = total_ms
    out["q1_rows_per_s"] = n / (total_ms * 1e-3)
    out["q1_packed_read_GBps"] = total_bytes / (total_ms * 1e-3) / 1e9
    out["note"] = ("one grouped scan per aggregated column over (value, group code); per-thread LDS bins (7 bins), one "
                   "partial per workgroup, k_group_final adds them; the reference's engine decodes every column first "
                   "(decode_only_ms per column) and then hashes 60 M rows on the CPU")
    ctx.close()
    return out


def q1_filtered_packed(adac, n=59_986_052):
    """Q1 with its WHERE clause on packed columns: q1_packed's columns plus an int32 l_shipdate in days.  One
    adac_scan_select_between (l_shipdate <= cutoff, about 98 % of the rows as in Q1) writes a selection bitmap, then one
    adac_scan_group_sum_valid per aggregated column under that bitmap; nothing is decoded.  Checked against numpy's
    GROUP BY over the kept rows before anything is timed.  Beside the masked time of every column: the unmasked
    adac_scan_group_sum of the same column in the same process, an all-ones and a 50 %-random bitmap, and what a
    bitmap costs the plain fused SUM (adac_scan_sum_valid with all ones over adac_scan_sum) on that column."""
    ctx = adac.Context(0)
    rng = np.random.default_rng(1992)
    cols = lineitem(rng, n, ("code", "l_quantity", "l_extendedprice", "l_partkey", "l_shipdate"))
    code, shipdate = cols.pop("code"), cols.pop("l_shipdate")
    cutoff = Q1_CUTOFF_DAY
    counts = adac.appender_segment_counts(n, 4)
    klay, kwords, kbytes, kwidths, _ = encode_column(adac, ctx, code, counts)
    dlay, dwords, dbytes, dwidths, _ = encode_column(adac, ctx, shipdate, counts)
    nw = (n + 63) // 64
    d_filter = ctx.alloc(nw * 8 + 8)
    d_selcnt = ctx.alloc(len(counts) * 8)
    select = lambda: dlay.scan_select_between(dwords, INT32_MIN_BITS, cutoff, d_filter, d_selcnt)
    select()
    ctx.sync()
    keep = shipdate <= cutoff
    assert int(d_selcnt.download(np.uint64, len(counts)).sum()) == int(keep.sum()), "filter parity"
    half = rng.random(n) < 0.5
    pad = np.zeros(nw * 64 - n, dtype=bool)
    d_half = ctx.upload(np.packbits(np.concatenate([half, pad]), bitorder="little").view(np.uint64))
    d_ones = ctx.upload(np.full(nw, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    d_sums, d_cnts = ctx.alloc(7 * 8), ctx.alloc(7 * 8)
    d_seg = ctx.alloc(len(counts) * 8)

    def grouped(v, m):
        bins = [(code == g) & m for g in range(6)] + [(code >= 6) & m]     # [6]: the overflow entry (empty here)
        return [int(v[b].astype(np.int64).sum()) & 0xFFFFFFFFFFFFFFFF for b in bins], [int(b.sum()) for b in bins]

    out = {"rows": n, "groups": 6, "cutoff_day": cutoff, "selected_rows": int(keep.sum()),
           "selected_fraction": float(keep.mean()), "key_widths": kwidths, "date_widths": dwidths,
           "filter_ms": timed(ctx, select), "filter_packed_bytes": dbytes, "columns": []}
    total_masked = total_plain = 0.0
    for name, v in cols.items():
        lay, words, nbytes, widths, _ = encode_column(adac, ctx, v, counts)
        for d_mask, m in ((d_filter, keep), (d_half, half), (d_ones, np.ones(n, dtype=bool)), (None, np.ones(n, dtype=bool))):
            lay.scan_group_sum_valid(words, klay, kwords, d_mask, 6, d_sums, d_cnts)
            ctx.sync()
            assert (d_sums.download(np.uint64, 7).tolist(), d_cnts.download(np.uint64, 7).tolist()) == grouped(v, m), "Q1 parity"
        ms_plain = timed(ctx, lambda: lay.scan_group_sum(words, klay, kwords, 6, d_sums, d_cnts))
        ms_filter = timed(ctx, lambda: lay.scan_group_sum_valid(words, klay, kwords, d_filter, 6, d_sums, d_cnts))
        ms_ones = timed(ctx, lambda: lay.scan_group_sum_valid(words, klay, kwords, d_ones, 6, d_sums, d_cnts))
        ms_half = timed(ctx, lambda: lay.scan_group_sum_valid(words, klay, kwords, d_half, 6, d_sums, d_cnts))
        ms_sum = timed(ctx, lambda: lay.scan_sum(words, d_seg))
        ms_sum_ones = timed(ctx, lambda: lay.scan_sum(words, d_seg, d_ones))
        total_masked += ms_filter
        total_plain += ms_plain
        out["columns"].append({"column": name, "widths": widths, "packed_bytes": nbytes,
                               "group_sum_ms": ms_plain, "group_sum_filtered_ms": ms_filter,
                               "group_sum_all_ones_ms": ms_ones, "group_sum_half_random_ms": ms_half,
                               "scan_sum_ms": ms_sum, "scan_sum_all_ones_ms": ms_sum_ones,
                               "grouped_mask_ratio": ms_ones / ms_plain, "fused_sum_mask_ratio": ms_sum_ones / ms_sum,
                               "ratio_gap": ms_ones / ms_plain - ms_sum_ones / ms_sum})
        del lay, words
    out["q1_filtered_ms"] = out["filter_ms"] + total_masked
    out["q1_unfiltered_three_aggregates_ms"] = total_plain
    out["note"] = ("q1_filtered = one selection scan over l_shipdate + three grouped scans under its bitmap; "
                   "grouped_mask_ratio = all-ones bitmap over no bitmap, fused_sum_mask_ratio = the same for the plain "
                   "fused SUM; the target is ratio_gap <= 0.10")
    ctx.close()
    return out


def q6_product_packed(adac, n=59_986_052):
    """TPC-H Q6 proper on packed columns: the four int32 columns and the three chained selects of q6_packed, then
    SUM(l_extendedprice * l_discount) under the final bitmap with adac_scan_sum_product — no value is materialised.
    Beside it, in the same process: what a caller paid before (adac_unpack of the two columns, after which the
    multiplication is still to do) and the two masked single-column SUMs, a lower bound for any walk of both columns."""
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1994), n, ("l_shipdate", "l_discount", "l_quantity", "l_extendedprice"))
    counts = adac.appender_segment_counts(n, 4)
    enc = {name: encode_column(adac, ctx, v, counts) for name, v in cols.items()}
    nw = (n + 63) // 64
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_cnt = ctx.alloc(len(counts) * 8)
    d_sum = ctx.alloc(len(counts) * 8)
    price, disc = enc["l_extendedprice"], enc["l_discount"]

    def selects():
        q6_selects(enc, bm, d_cnt)

    def product():
        price.lay.scan_sum_product(price.words, disc.lay, disc.words, d_sum, bm[2])

    def q6():
        selects()
        product()

    q6()
    ctx.sync()
    m = q6_mask(cols)
    want = int((cols["l_extendedprice"][m].astype(np.int64) * cols["l_discount"][m]).sum())
    assert int(d_sum.download(np.uint64, len(counts)).sum(dtype=np.uint64)) == want, "Q6 parity"
    assert int(d_cnt.download(np.uint64, len(counts)).sum()) == int(m.sum())
    d_out = ctx.alloc(n * 4 + 64)

    def unpack_two():
        price.lay.unpack(price.words, d_out)
        disc.lay.unpack(disc.words, d_out)

    def two_sums():
        price.lay.scan_sum(price.words, d_sum, bm[2])
        disc.lay.scan_sum(disc.words, d_sum, bm[2])

    ms = {}
    for name, fn in (("q6_product_on_packed", q6), ("select_chain", selects), ("sum_product_masked", product),
                     ("unpack_price_and_discount", unpack_two), ("two_masked_scan_sums", two_sums),
                     ("sum_product_unmasked", lambda: price.lay.scan_sum_product(price.words, disc.lay, disc.words, d_sum))):
        ms[name] = timed(ctx, fn)
    product()  # leave the masked result behind and check it once more after the timed loops
    assert int(d_sum.download(np.uint64, len(counts)).sum(dtype=np.uint64)) == want, "Q6 parity (after timing)"
    two = price.nbytes + disc.nbytes
    out = {"rows": n, "selected_rows": int(m.sum()), "widths": {k: e.widths for k, e in enc.items()},
           "packed_bytes": {k: e.nbytes for k, e in enc.items()}, "step_ms": ms,
           "sum_product_packed_read_GBps": (two + n / 8) / (ms["sum_product_masked"] * 1e-3) / 1e9,
           "unpack_two_columns_total_GBps": (two + 2 * n * 4) / (ms["unpack_price_and_discount"] * 1e-3) / 1e9,
           "product_faster_than_unpack": ms["sum_product_masked"] < ms["unpack_price_and_discount"],
           "groups_by_form": product_form_groups(price.descs, disc.descs),
           "note": "sum_product_masked = adac_scan_sum_product(l_extendedprice, l_discount) under the final bitmap of the "
                   "three chained selects; unpack_price_and_discount is what a caller paid before it could start to "
                   "multiply; two_masked_scan_sums is a lower bound for any walk of the two columns"}
    ctx.close()
    return out


def q6_bitpacking(adac, n=59_986_052):
    """TPC-H Q6 end to end on DuckDB's own BITPACKING blocks: q6_product_packed's four int32 columns compressed the way
    bitpacking_fused_scans builds its columns, the three chained adac_bp_scan_select_between calls, then
    adac_bp_scan_sum_product(l_extendedprice, l_discount) under the final bitmap — checked against numpy.  Beside it, in
    the same process and interleaved: adac_bp_unpack of the two columns the product reads (what a caller paid before it
    could start to multiply).  Second line: adac_bp_scan_group_sum of l_quantity by a 6-valued uint8 code column under
    Q1's bitmap (l_shipdate <= cutoff), against adac_bp_unpack of those two columns."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1994), n, ("l_shipdate", "l_discount", "l_quantity", "l_extendedprice", "code"))
    enc = {name: bitpacking_blocks(adac, ctx, bp.Compressed(v), v.dtype) for name, v in cols.items()}
    nw = (n + 63) // 64
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_q1 = ctx.alloc(nw * 8 + 8)
    price, disc, qty, ship, code = (enc[k] for k in ("l_extendedprice", "l_discount", "l_quantity", "l_shipdate", "code"))
    d_cnt = ctx.alloc(max(e.nseg for e in enc.values()) * 8)
    d_sum = ctx.alloc(price.nseg * 8)
    d_gsum, d_gcnt = ctx.alloc(7 * 8), ctx.alloc(7 * 8)
    cutoff = Q1_CUTOFF_DAY

    def selects():
        q6_selects(enc, bm, d_cnt)

    def product():
        price.lay.scan_sum_product(price.words, disc.lay, disc.words, d_sum, bm[2])

    def q6():
        selects()
        product()

    def grouped():
        qty.lay.scan_group_sum(qty.words, code.lay, code.words, 6, d_gsum, d_gcnt, d_q1)

    q6()
    ship.lay.scan_select_between(ship.words, INT32_MIN_BITS, cutoff, d_q1, d_cnt)
    grouped()
    ctx.sync()
    m = q6_mask(cols)
    want_q6 = int((cols["l_extendedprice"][m].astype(np.int64) * cols["l_discount"][m]).sum())
    assert int(d_sum.download(np.uint64, price.nseg).sum(dtype=np.uint64)) == want_q6, "Q6 parity"
    keep = cols["l_shipdate"] <= cutoff
    want_gs = np.bincount(cols["code"][keep], weights=None, minlength=7).astype(np.uint64)
    want_sum = np.zeros(7, dtype=np.int64)
    np.add.at(want_sum, cols["code"][keep], cols["l_quantity"][keep].astype(np.int64))
    assert np.array_equal(d_gcnt.download(np.uint64, 7), want_gs), "grouped COUNT parity"
    assert np.array_equal(d_gsum.download(np.uint64, 7), want_sum.view(np.uint64)), "grouped SUM parity"
    d_out = ctx.alloc(n * 4 + 64)

    def unpack_price_disc():
        price.lay.unpack(price.words, d_out)
        disc.lay.unpack(disc.words, d_out)

    def unpack_qty_code():
        qty.lay.unpack(qty.words, d_out)
        code.lay.unpack(code.words, d_out)

    ms = {}
    for name, fn in (("q6_on_bitpacking", q6), ("select_chain", selects), ("sum_product_masked", product),
                     ("unpack_price_and_discount", unpack_price_disc),
                     ("sum_product_unmasked", lambda: price.lay.scan_sum_product(price.words, disc.lay, disc.words, d_sum)),
                     ("group_sum_masked", grouped), ("unpack_quantity_and_code", unpack_qty_code),
                     ("sum_product_masked_again", product), ("unpack_price_and_discount_again", unpack_price_disc),
                     ("group_sum_masked_again", grouped), ("unpack_quantity_and_code_again", unpack_qty_code)):
        ms[name] = timed(ctx, fn)
    product()  # leave the masked results behind and check them once more after the timed loops
    grouped()
    assert int(d_sum.download(np.uint64, price.nseg).sum(dtype=np.uint64)) == want_q6, "Q6 parity (after timing)"
    assert np.array_equal(d_gcnt.download(np.uint64, 7), want_gs), "grouped COUNT parity (after timing)"
    prod = min(ms["sum_product_masked"], ms["sum_product_masked_again"])
    dec = min(ms["unpack_price_and_discount"], ms["unpack_price_and_discount_again"])
    grp = min(ms["group_sum_masked"], ms["group_sum_masked_again"])
    dec2 = min(ms["unpack_quantity_and_code"], ms["unpack_quantity_and_code_again"])
    two = price.nbytes + disc.nbytes
    out = {"rows": n, "selected_rows": int(m.sum()), "q1_selected_rows": int(keep.sum()),
           "columns": {k: e.info for k, e in enc.items()},
           "packed_bytes": {k: e.nbytes for k, e in enc.items()}, "step_ms": ms,
           "sum_product_masked_ms": prod, "unpack_price_and_discount_ms": dec, "sum_product_over_decode": prod / dec,
           "group_sum_masked_ms": grp, "unpack_quantity_and_code_ms": dec2, "group_sum_over_decode": grp / dec2,
           "sum_product_packed_read_GBps": (two + n / 8) / (prod * 1e-3) / 1e9,
           "unpack_two_columns_total_GBps": (two + 2 * n * 4) / (dec * 1e-3) / 1e9,
           "note": "sum_product_masked = adac_bp_scan_sum_product(l_extendedprice, l_discount) under the final bitmap of "
                   "the three chained adac_bp_scan_select_between calls; group_sum_masked = adac_bp_scan_group_sum("
                   "l_quantity BY code, 6 groups) under l_shipdate <= cutoff; the decodes are adac_bp_unpack of the two "
                   "columns each call reads; every *_over_decode takes the faster of two interleaved timings of each"}
    ctx.close()
    return out


Q12_RECEIPT_DATES = (8766, 9130)   # l_receiptdate in 1994


def q12_bitpacking(adac, n=59_986_052):
    """TPC-H Q12's WHERE clause on DuckDB's own BITPACKING blocks, three int32 day columns: l_receiptdate BETWEEN one
    year (adac_bp_scan_select_between), then l_commitdate < l_receiptdate under that bitmap and l_shipdate <
    l_commitdate under that one (adac_bp_scan_select_compare); the final bitmap and counts checked against numpy before
    and after the timing.  Interleaved in the same process: the chain; the BETWEEN; each compare in the chain and alone
    (no validity); adac_bp_scan_count_compare; adac_bp_unpack of the two columns each compare reads;
    adac_bp_scan_sum_product on the same pair, the pair walk that was there before."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1994), n, ("l_shipdate", "l_commitdate", "l_receiptdate"))
    enc = {name: bitpacking_blocks(adac, ctx, bp.Compressed(v), v.dtype) for name, v in cols.items()}
    ship, commit, receipt = (enc[k] for k in ("l_shipdate", "l_commitdate", "l_receiptdate"))
    nw = (n + 63) // 64
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_alone = ctx.alloc(nw * 8 + 8)
    nseg = max(e.nseg for e in enc.values())
    d_cnt, d_final, d_sum = ctx.alloc(nseg * 8), ctx.alloc(nseg * 8), ctx.alloc(nseg * 8)
    d_out = ctx.alloc(n * 4 + 64)
    LT = adac.CMP_LT
    pairs = {"commit_lt_receipt": (commit, receipt, bm[0], bm[1], d_cnt), "ship_lt_commit": (ship, commit, bm[1], bm[2], d_final)}

    def between():
        receipt.lay.scan_select_between(receipt.words, *Q12_RECEIPT_DATES, bm[0], d_cnt)

    def compare(name, masked):
        a, b, d_valid, d_bitmap, d_counts = pairs[name]
        if masked:
            return lambda: a.lay.scan_select_compare(a.words, b.lay, b.words, LT, d_bitmap, d_counts, d_valid)
        return lambda: a.lay.scan_select_compare(a.words, b.lay, b.words, LT, d_alone, d_cnt)

    def count(name):
        a, b = pairs[name][:2]
        return lambda: a.lay.scan_count_compare(a.words, b.lay, b.words, LT, d_cnt)

    def unpack(name):
        a, b = pairs[name][:2]

        def both():
            a.lay.unpack(a.words, d_out)
            b.lay.unpack(b.words, d_out)
        return both

    def product(name):
        a, b = pairs[name][:2]
        return lambda: a.lay.scan_sum_product(a.words, b.lay, b.words, d_sum)

    def chain():
        between()
        compare("commit_lt_receipt", True)()
        compare("ship_lt_commit", True)()

    m1 = (cols["l_receiptdate"] >= Q12_RECEIPT_DATES[0]) & (cols["l_receiptdate"] <= Q12_RECEIPT_DATES[1])
    m2 = m1 & (cols["l_commitdate"] < cols["l_receiptdate"])
    m3 = m2 & (cols["l_shipdate"] < cols["l_commitdate"])
    full = np.zeros(nw * 64, dtype=bool)
    full[:n] = m3
    want_words = np.packbits(full, bitorder="little").view(np.uint64)
    starts = np.concatenate([[0], np.cumsum(ship.counts[:-1], dtype=np.int64)])
    want_counts = np.add.reduceat(m3.astype(np.uint64), starts)

    def parity(when):
        chain()
        ctx.sync()
        assert np.array_equal(bm[2].download(np.uint64, nw), want_words), "Q12 bitmap parity (%s)" % when
        assert np.array_equal(d_final.download(np.uint64, ship.nseg), want_counts), "Q12 counts parity (%s)" % when

    parity("before timing")
    entries = [("q12_where_chain", chain), ("select_between_receiptdate", between)]
    for name in pairs:
        entries += [(name + "_in_chain", compare(name, True)), (name + "_alone", compare(name, False)),
                    (name + "_count", count(name)), (name + "_unpack_two_columns", unpack(name)),
                    (name + "_sum_product", product(name))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    out = {"rows": n, "selected_rows": {"receiptdate_in_year": int(m1.sum()), "and_commit_lt_receipt": int(m2.sum()),
                                        "and_ship_lt_commit": int(m3.sum())},
           "columns": {k: e.info for k, e in enc.items()}, "packed_bytes": {k: e.nbytes for k, e in enc.items()},
           "ms": med, "q12_where_chain_ms": med["q12_where_chain"],
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()}}
    for name, (a, b, _, _, _) in pairs.items():
        sel, dec, prod = med[name + "_alone"], med[name + "_unpack_two_columns"], med[name + "_sum_product"]
        two = a.nbytes + b.nbytes
        out[name] = {"select_alone_ms": sel, "select_in_chain_ms": med[name + "_in_chain"], "count_ms": med[name + "_count"],
                     "unpack_two_columns_ms": dec, "sum_product_ms": prod, "select_over_decode": sel / dec,
                     "select_in_chain_over_decode": med[name + "_in_chain"] / dec,
                     "count_over_decode": med[name + "_count"] / dec, "select_over_sum_product": sel / prod,
                     "count_over_sum_product": med[name + "_count"] / prod,
                     "select_packed_read_GBps": two / (sel * 1e-3) / 1e9, "bitmap_bytes_written": nw * 8,
                     "sum_product_packed_read_GBps": two / (prod * 1e-3) / 1e9,
                     "unpack_two_columns_total_GBps": (two + 2 * n * 4) / (dec * 1e-3) / 1e9}
        print("q12_bitpacking %s: select %.4f ms (in chain %.4f, count %.4f), decode of both %.4f, sum_product %.4f" %
              (name, sel, med[name + "_in_chain"], med[name + "_count"], dec, prod), file=sys.stderr, flush=True)
    out["note"] = ("l_commitdate and l_receiptdate are independent uniform draws in l_shipdate's range: dbgen's dates are "
                   "correlated and select fewer rows.  *_alone = adac_bp_scan_select_compare(LT) with d_validity NULL, "
                   "*_in_chain = the same call under the previous step's bitmap, *_count = adac_bp_scan_count_compare "
                   "with d_validity NULL, *_unpack_two_columns = adac_bp_unpack of the two columns the compare reads, "
                   "*_sum_product = adac_bp_scan_sum_product on the same pair without a mask; medians of %d interleaved "
                   "rounds of %d calls each" % (ROUNDS, INNER))
    ctx.close()
    return out


def q12_packed(adac, n=59_986_052):
    """TPC-H Q12's WHERE clause on columns packed by adac_encode — q12_bitpacking's table (same seed, same three int32
    day columns) on the succinct codec: l_receiptdate BETWEEN one year (adac_scan_select_between), then l_commitdate <
    l_receiptdate under that bitmap and l_shipdate < l_commitdate under that one (adac_scan_select_compare); the final
    counts checked against numpy before and after the timing.  Interleaved in the same process, for commit < receipt:
    the compare alone and in the chain, adac_scan_count_compare, adac_unpack of the same two columns,
    adac_scan_sum_product on the same pair, and adac_bp_scan_select_compare on the same two columns as BITPACKING
    blocks.  A second cell, "sorted": the table sorted by l_receiptdate with l_commitdate = l_receiptdate - U[70, 100]
    days (clustered with the sort key), so that the two segments' value intervals are disjoint in most scan groups and
    the compare is answered from the descriptors (the header form)."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    cols = lineitem(np.random.default_rng(1994), n, ("l_shipdate", "l_commitdate", "l_receiptdate"))
    counts = adac.appender_segment_counts(n, 4)
    nseg, nw = len(counts), (n + 63) // 64
    LT = adac.CMP_LT
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_alone = ctx.alloc(nw * 8 + 8)
    d_cnt, d_final, d_sum = ctx.alloc(nseg * 8), ctx.alloc(nseg * 8), ctx.alloc(nseg * 8)
    d_out = ctx.alloc(n * 4 + 64)
    starts = np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.int64)])

    def select(a, b, d_bitmap, d_counts, d_valid=None):
        a.lay.scan_select_compare(a.words, b.lay, b.words, LT, d_bitmap, d_counts, d_valid)

    # ---- the table as drawn
    enc = {name: encode_column(adac, ctx, v, counts) for name, v in cols.items()}
    ship, commit, receipt = (enc[k] for k in ("l_shipdate", "l_commitdate", "l_receiptdate"))

    def between():
        receipt.lay.scan_select_between(receipt.words, *Q12_RECEIPT_DATES, bm[0], d_cnt)

    def chain():
        between()
        select(commit, receipt, bm[1], d_cnt, bm[0])
        select(ship, commit, bm[2], d_final, bm[1])

    def unpack_two():
        commit.lay.unpack(commit.words, d_out)
        receipt.lay.unpack(receipt.words, d_out)

    m1 = (cols["l_receiptdate"] >= Q12_RECEIPT_DATES[0]) & (cols["l_receiptdate"] <= Q12_RECEIPT_DATES[1])
    m2 = m1 & (cols["l_commitdate"] < cols["l_receiptdate"])
    m3 = m2 & (cols["l_shipdate"] < cols["l_commitdate"])
    want_counts = np.add.reduceat(m3.astype(np.uint64), starts)

    def parity(when):
        chain()
        ctx.sync()
        assert np.array_equal(d_final.download(np.uint64, nseg), want_counts), "Q12 counts parity (%s)" % when
        full = np.zeros(nw * 64, dtype=bool)
        full[:n] = m3
        assert np.array_equal(bm[2].download(np.uint64, nw), np.packbits(full, bitorder="little").view(np.uint64)), \
            "Q12 bitmap parity (%s)" % when

    parity("before timing")
    blocks = {k: bitpacking_blocks(adac, ctx, bp.Compressed(cols[k]), cols[k].dtype) for k in ("l_commitdate", "l_receiptdate")}
    bc, br = blocks["l_commitdate"], blocks["l_receiptdate"]
    d_bcnt = ctx.alloc(max(bc.nseg, br.nseg) * 8)

    # ---- the sorted table
    order = np.argsort(cols["l_receiptdate"], kind="stable")
    s_receipt = cols["l_receiptdate"][order]
    s_commit = (s_receipt - np.random.default_rng(1995).integers(70, 101, size=n)).astype(np.int32)
    del order
    srt = {"l_commitdate": encode_column(adac, ctx, s_commit, counts), "l_receiptdate": encode_column(adac, ctx, s_receipt, counts)}
    sc, sr = srt["l_commitdate"], srt["l_receiptdate"]
    select(sc, sr, d_alone, d_cnt)
    ctx.sync()
    assert int(d_cnt.download(np.uint64, nseg).sum()) == n, "sorted cell: every commit date is before its receipt date"
    select(sr, sc, d_alone, d_cnt)
    ctx.sync()
    assert int(d_cnt.download(np.uint64, nseg).sum()) == 0

    def census(a, b):
        fs = forms.compare_form_groups(a.descs, b.descs)
        return {f: fs.count(f) for f in ("header", "fast", "generic")}

    entries = [("q12_where_chain", chain), ("select_between_receiptdate", between),
               ("compare_alone", lambda: select(commit, receipt, d_alone, d_cnt)),
               ("compare_in_chain", lambda: select(commit, receipt, bm[1], d_cnt, bm[0])),
               ("count_compare", lambda: commit.lay.scan_count_compare(commit.words, receipt.lay, receipt.words, LT, d_cnt)),
               ("unpack_two_columns", unpack_two),
               ("sum_product", lambda: commit.lay.scan_sum_product(commit.words, receipt.lay, receipt.words, d_sum)),
               ("bp_select_compare", lambda: bc.lay.scan_select_compare(bc.words, br.lay, br.words, LT, d_alone, d_bcnt)),
               ("sorted_compare_alone", lambda: select(sc, sr, d_alone, d_cnt)),
               ("sorted_count_compare", lambda: sc.lay.scan_count_compare(sc.words, sr.lay, sr.words, LT, d_cnt)),
               ("sorted_sum_product", lambda: sc.lay.scan_sum_product(sc.words, sr.lay, sr.words, d_sum))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    two, stwo = commit.nbytes + receipt.nbytes, sc.nbytes + sr.nbytes
    out = {"rows": n, "segments": nseg,
           "selected_rows": {"receiptdate_in_year": int(m1.sum()), "and_commit_lt_receipt": int(m2.sum()),
                             "and_ship_lt_commit": int(m3.sum())},
           "widths": {k: e.widths for k, e in enc.items()}, "packed_bytes": {k: e.nbytes for k, e in enc.items()},
           "bitpacking_bytes": {k: e.nbytes for k, e in blocks.items()},
           "segment_pairs_by_form": census(commit, receipt),
           "ms": med, "q12_where_chain_ms": med["q12_where_chain"],
           "commit_lt_receipt": {
               "select_alone_ms": med["compare_alone"], "select_in_chain_ms": med["compare_in_chain"],
               "count_ms": med["count_compare"], "unpack_two_columns_ms": med["unpack_two_columns"],
               "sum_product_ms": med["sum_product"], "bp_select_compare_ms": med["bp_select_compare"],
               "select_over_decode": med["compare_alone"] / med["unpack_two_columns"],
               "select_over_sum_product": med["compare_alone"] / med["sum_product"],
               "count_over_sum_product": med["count_compare"] / med["sum_product"],
               "select_over_bp_select": med["compare_alone"] / med["bp_select_compare"],
               "select_packed_read_GBps": two / (med["compare_alone"] * 1e-3) / 1e9, "bitmap_bytes_written": nw * 8,
               "sum_product_packed_read_GBps": two / (med["sum_product"] * 1e-3) / 1e9},
           "sorted": {"widths": {k: e.widths for k, e in srt.items()}, "packed_bytes": {k: e.nbytes for k, e in srt.items()},
                      "segment_pairs_by_form": census(sc, sr), "select_alone_ms": med["sorted_compare_alone"],
                      "count_ms": med["sorted_count_compare"], "sum_product_ms": med["sorted_sum_product"],
                      "select_over_sum_product": med["sorted_compare_alone"] / med["sorted_sum_product"],
                      "packed_bytes_not_read": stwo},
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()},
           "note": ("l_commitdate and l_receiptdate are independent uniform draws in l_shipdate's range (dbgen's dates are "
                    "correlated and select fewer rows).  compare_alone = adac_scan_select_compare(LT) with d_validity NULL, "
                    "compare_in_chain = the same call under the BETWEEN's bitmap, count_compare = adac_scan_count_compare, "
                    "unpack_two_columns = adac_unpack of the two columns, sum_product = adac_scan_sum_product on the same "
                    "pair without a mask, bp_select_compare = adac_bp_scan_select_compare on the same two columns as "
                    "BITPACKING blocks.  sorted: the table sorted by l_receiptdate, l_commitdate = l_receiptdate - U[70, 100] "
                    "days.  Medians of %d interleaved rounds of %d calls each" % (ROUNDS, INNER))}
    print("q12_packed commit<receipt: select %.4f ms (in chain %.4f, count %.4f), decode of both %.4f, sum_product %.4f, "
          "bp select %.4f; sorted: select %.4f, sum_product %.4f" %
          (med["compare_alone"], med["compare_in_chain"], med["count_compare"], med["unpack_two_columns"],
           med["sum_product"], med["bp_select_compare"], med["sorted_compare_alone"], med["sorted_sum_product"]),
          file=sys.stderr, flush=True)
    ctx.close()
    return out


Q4_ORDER_DATES = (8582, 8673)   # o_orderdate in 1993-07-01 .. 1993-09-30, one quarter


def q4_packed(adac, n_orders=15_000_000):
    """TPC-H Q4 end to end on packed columns, a semi-join through a bit set indexed by the key: adac_scan_select_between
    on o_orderdate for one quarter, adac_scan_select_compare on l_commitdate < l_receiptdate, adac_scan_build_member over
    l_orderkey under that bitmap (the key set), adac_scan_select_member over o_orderkey under the date bitmap, and
    adac_scan_group_sum_valid for the counts per o_orderpriority; the five counts checked against numpy (np.isin) before
    and after the timing.  Synthetic orders at SF10 size: o_orderkey sparse-increasing as dbgen's (8 keys used of every
    32), one to seven lineitems per order, o_orderpriority a 5-valued uint8 code, o_orderdate an int32 day.  Interleaved
    in the same process, for the probe (o_orderkey) and for the build (l_orderkey): adac_scan_select_between on the same
    column (the same packed bytes: the floor), adac_scan_sum of it (the key columns are sorted, so the BETWEEN skips the
    segments that lie outside its range on their descriptors; the SUM reads every packed byte) and
    adac_unpack of the column (what the call replaces).  A second cell,
    "q12_shipmode": Q12's l_shipmode IN ('MAIL', 'SHIP') as a probe of a two-member set on a 7-valued uint8 code."""
    ctx = adac.Context(0)
    rng = np.random.default_rng(1993)
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)
    del idx
    o_priority = rng.integers(0, 5, size=n_orders).astype(np.uint8)
    o_orderdate = rng.integers(8036, 10562 - 151, size=n_orders).astype(np.int32)
    l_orderkey = np.repeat(o_orderkey, rng.integers(1, 8, size=n_orders))
    n = len(l_orderkey)
    dates = lineitem(rng, n, ("l_commitdate", "l_receiptdate"))
    oc, lc = adac.appender_segment_counts(n_orders, 4), adac.appender_segment_counts(n, 4)
    oseg, lseg, ow, lw = len(oc), len(lc), (n_orders + 63) // 64, (n + 63) // 64
    okey, odate = encode_column(adac, ctx, o_orderkey, oc), encode_column(adac, ctx, o_orderdate, oc)
    oprio = encode_column(adac, ctx, o_priority, oc)
    lkey = encode_column(adac, ctx, l_orderkey, lc)
    commit, receipt = (encode_column(adac, ctx, dates[k], lc) for k in ("l_commitdate", "l_receiptdate"))
    base, bits = 1, int(o_orderkey.max())
    sw = (bits + 63) // 64
    d_set, d_set2 = ctx.alloc(sw * 8 + 8), ctx.alloc(sw * 8 + 8)
    bm_l, bm_od, bm_o, bm_x = ctx.alloc(lw * 8 + 8), ctx.alloc(ow * 8 + 8), ctx.alloc(ow * 8 + 8), ctx.alloc(lw * 8 + 8)
    d_lcnt, d_ocnt = ctx.alloc(lseg * 8), ctx.alloc(oseg * 8)
    d_lsum, d_osum = ctx.alloc(lseg * 8), ctx.alloc(oseg * 8)
    d_sums, d_gcnt = ctx.alloc(6 * 8), ctx.alloc(6 * 8)
    d_out = ctx.alloc(n * 4 + 64)

    def chain():
        odate.lay.scan_select_between(odate.words, *Q4_ORDER_DATES, bm_od, d_ocnt)
        commit.lay.scan_select_compare(commit.words, receipt.lay, receipt.words, adac.CMP_LT, bm_l, d_lcnt)
        lkey.lay.scan_build_member(lkey.words, base, bits, d_set, d_lcnt, bm_l)
        okey.lay.scan_select_member(okey.words, d_set, base, bits, bm_o, d_ocnt, bm_od)
        okey.lay.scan_group_sum_valid(okey.words, oprio.lay, oprio.words, bm_o, 5, d_sums, d_gcnt)

    late = dates["l_commitdate"] < dates["l_receiptdate"]
    in_quarter = (o_orderdate >= Q4_ORDER_DATES[0]) & (o_orderdate <= Q4_ORDER_DATES[1])
    exists = np.isin(o_orderkey, l_orderkey[late])
    want = np.bincount(o_priority[in_quarter & exists], minlength=5)

    def parity(when):
        chain()
        ctx.sync()
        got = d_gcnt.download(np.uint64, 6)
        assert [int(x) for x in got] == [int(x) for x in want] + [0], "Q4 counts parity (%s): %s" % (when, got)

    parity("before timing")
    # Q12's ship mode: a 7-valued code, two members
    shipmode = rng.integers(0, 7, size=n).astype(np.uint8)
    mcounts = adac.appender_segment_counts(n, 1)
    mode = encode_column(adac, ctx, shipmode, mcounts)
    d_mcnt, d_msum = ctx.alloc(len(mcounts) * 8), ctx.alloc(len(mcounts) * 8)
    d_inlist = ctx.upload(np.array([(1 << 2) | (1 << 5)], dtype=np.uint64))
    mode.lay.scan_count_member(mode.words, d_inlist, 0, 7, d_mcnt)
    ctx.sync()
    in_list = int(np.isin(shipmode, [2, 5]).sum())
    assert int(d_mcnt.download(np.uint64, len(mcounts)).sum()) == in_list, "Q12 ship mode parity"

    key_lo, key_hi = 1, bits // 2
    entries = [("q4_chain", chain),
               ("probe_select_member", lambda: okey.lay.scan_select_member(okey.words, d_set, base, bits, bm_o, d_ocnt)),
               ("probe_select_member_in_chain",
                lambda: okey.lay.scan_select_member(okey.words, d_set, base, bits, bm_o, d_ocnt, bm_od)),
               ("probe_count_member", lambda: okey.lay.scan_count_member(okey.words, d_set, base, bits, d_ocnt)),
               ("probe_select_between", lambda: okey.lay.scan_select_between(okey.words, key_lo, key_hi, bm_o, d_ocnt)),
               ("probe_scan_sum", lambda: okey.lay.scan_sum(okey.words, d_osum)),
               ("probe_unpack", lambda: okey.lay.unpack(okey.words, d_out)),
               ("build_member", lambda: lkey.lay.scan_build_member(lkey.words, base, bits, d_set2, d_lcnt)),
               ("build_member_in_chain", lambda: lkey.lay.scan_build_member(lkey.words, base, bits, d_set2, d_lcnt, bm_l)),
               ("build_select_between", lambda: lkey.lay.scan_select_between(lkey.words, key_lo, key_hi, bm_x, d_lcnt)),
               ("build_scan_sum", lambda: lkey.lay.scan_sum(lkey.words, d_lsum)),
               ("build_unpack", lambda: lkey.lay.unpack(lkey.words, d_out)),
               ("shipmode_select_member", lambda: mode.lay.scan_select_member(mode.words, d_inlist, 0, 7, bm_x, d_mcnt)),
               ("shipmode_count_member", lambda: mode.lay.scan_count_member(mode.words, d_inlist, 0, 7, d_mcnt)),
               ("shipmode_select_between", lambda: mode.lay.scan_select_between(mode.words, 2, 5, bm_x, d_mcnt)),
               ("shipmode_scan_sum", lambda: mode.lay.scan_sum(mode.words, d_msum)),
               ("shipmode_unpack", lambda: mode.lay.unpack(mode.words, d_out))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    kind32 = (4, True)

    def census(e, kind, b, nb):
        fs = forms.member_form_groups(e.descs, kind, b, nb)
        return {f: fs.count(f) for f in sorted(set(fs) - {None})}

    def cell(prefix, call, e):
        return {"ms": med[call], "select_between_ms": med[prefix + "_select_between"],
                "scan_sum_ms": med[prefix + "_scan_sum"], "unpack_ms": med[prefix + "_unpack"],
                "over_select_between": med[call] / med[prefix + "_select_between"],
                "over_scan_sum": med[call] / med[prefix + "_scan_sum"],
                "over_unpack": med[call] / med[prefix + "_unpack"],
                "packed_read_GBps": e.nbytes / (med[call] * 1e-3) / 1e9}

    out = {"orders": n_orders, "lineitems": n, "set_bits": bits, "set_bytes": sw * 8,
           "selected": {"lineitems_commit_lt_receipt": int(late.sum()), "orders_in_quarter": int(in_quarter.sum()),
                        "orders_with_a_late_lineitem": int(exists.sum()), "orders_counted": int(want.sum())},
           "counts_by_priority": [int(x) for x in want],
           "widths": {"o_orderkey": okey.widths, "l_orderkey": lkey.widths, "o_orderdate": odate.widths,
                      "o_orderpriority": oprio.widths, "l_shipmode": mode.widths},
           "packed_bytes": {"o_orderkey": okey.nbytes, "l_orderkey": lkey.nbytes, "l_shipmode": mode.nbytes},
           "segments_by_form": {"probe_o_orderkey": census(okey, kind32, base, bits),
                                "build_l_orderkey": census(lkey, kind32, base, bits),
                                "q12_shipmode": census(mode, (1, False), 0, 7)},
           "ms": med, "q4_chain_ms": med["q4_chain"],
           "probe": dict(cell("probe", "probe_select_member", okey), in_chain_ms=med["probe_select_member_in_chain"],
                         count_ms=med["probe_count_member"]),
           "build": dict(cell("build", "build_member", lkey), in_chain_ms=med["build_member_in_chain"]),
           "q12_shipmode": dict(cell("shipmode", "shipmode_select_member", mode), count_ms=med["shipmode_count_member"],
                                rows_in_list=in_list),
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()},
           "note": ("Synthetic orders / lineitem at SF10 size; l_commitdate and l_receiptdate are independent uniform draws. "
                    "probe_* on o_orderkey, build_* on l_orderkey, shipmode_* on a 7-valued uint8 code over the lineitem "
                    "rows; *_select_between = adac_scan_select_between on the same column (lower half of the keys; codes "
                    "2 .. 5; on the sorted key columns it skips the segments outside the range on their "
                    "descriptors), *_scan_sum = adac_scan_sum of the column (reads every packed byte), *_unpack = adac_unpack "
                    "of the column; *_in_chain = the call under the chain's bitmap.  "
                    "Medians of %d interleaved rounds of %d calls each" % (ROUNDS, INNER))}
    print("q4_packed chain %.4f ms; " % med["q4_chain"] + "; ".join(
        "%s %.4f (between %.4f, sum %.4f, unpack %.4f)" % (name, med[call], med[p + "_select_between"], med[p + "_scan_sum"],
                                                          med[p + "_unpack"])
        for name, call, p in (("probe", "probe_select_member", "probe"), ("build", "build_member", "build"),
                              ("ship mode", "shipmode_select_member", "shipmode"))), file=sys.stderr, flush=True)
    ctx.close()
    return out


Q18_QUANTITY = 300   # HAVING SUM(l_quantity) > 300


def q18_packed(adac, n_orders=15_000_000):
    """TPC-H Q18's aggregate on packed columns: SUM(l_quantity) GROUP BY l_orderkey as adac_scan_group_sum_dense over the
    dense domain of the order keys, then HAVING SUM > 300 and the orders: adac_encode of the sums as a UINT64 layout,
    adac_scan_select_between for > 300, and that bitmap as the d_set of adac_scan_select_member over o_orderkey; the
    qualifying orders checked against numpy before and after the timing.  Synthetic tables at SF10 size as in q4_packed:
    o_orderkey sparse-increasing (8 keys used of every 32), one to seven lineitems per order, l_quantity 1 .. 50.
    Interleaved in the same process: the sum with and without d_counts at group_dense_combine 1 and 0, the count entry,
    adac_scan_build_member over the same key column and adac_unpack of the two columns (the comparison points), the same
    sum with the rows shuffled (no runs), GROUP BY l_shipdate over all days, and over one year of days (a domain of 365
    keys: the window form) with the window on and off (group_dense_window)."""
    ctx = adac.Context(0)
    rng = np.random.default_rng(1998)
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)
    del idx
    l_orderkey = np.repeat(o_orderkey, rng.integers(1, 8, size=n_orders))
    n = len(l_orderkey)
    cols = lineitem(rng, n, ("l_quantity", "l_shipdate"))
    perm = rng.permutation(n)
    oc, lc = adac.appender_segment_counts(n_orders, 4), adac.appender_segment_counts(n, 4)
    okey = encode_column(adac, ctx, o_orderkey, oc)
    lkey, qty = encode_column(adac, ctx, l_orderkey, lc), encode_column(adac, ctx, cols["l_quantity"], lc)
    skey, sqty = encode_column(adac, ctx, l_orderkey[perm], lc), encode_column(adac, ctx, cols["l_quantity"][perm], lc)
    ship = encode_column(adac, ctx, cols["l_shipdate"], lc)
    base, span = 1, int(o_orderkey.max())
    day0, days = 8036, 10562 - 8036
    year0, year = 8766, 365   # 1994
    sw, ow, lseg, oseg = (span + 63) // 64, (n_orders + 63) // 64, len(lc), len(oc)
    d_sums, d_counts, d_sums2 = ctx.alloc(span * 8), ctx.alloc(span * 8), ctx.alloc(span * 8)
    d_day_sums = ctx.alloc(days * 8)
    d_set, d_lcnt, d_ocnt = ctx.alloc(sw * 8 + 8), ctx.alloc(lseg * 8), ctx.alloc(oseg * 8)
    bm_o = ctx.alloc(ow * 8 + 8)
    d_out = ctx.alloc(n * 4 + 64)
    sc = adac.appender_segment_counts(span, 8)
    slay = adac.Layout(ctx, np.uint64, sc)
    d_swords, d_scnt = ctx.alloc(slay.max_arena_words * 8 + 16).zero(), ctx.alloc(len(sc) * 8)

    def sums(k=lkey, v=qty, counts=None, out=d_sums):
        k.lay.scan_group_sum_dense(k.words, v.lay, v.words, base, span, out, counts, d_lcnt)

    def chain():
        sums()
        slay.encode(d_sums, d_swords)
        slay.scan_select_between(d_swords, Q18_QUANTITY + 1, 0xFFFFFFFFFFFFFFFF, d_set, d_scnt)
        okey.lay.scan_select_member(okey.words, d_set, base, span, bm_o, d_ocnt)

    want_sums = np.bincount(l_orderkey - base, weights=cols["l_quantity"], minlength=span).astype(np.uint64)
    large = want_sums[(o_orderkey - base).astype(np.int64)] > Q18_QUANTITY
    want_days = np.bincount(cols["l_shipdate"] - day0, weights=cols["l_quantity"], minlength=days).astype(np.uint64)

    def parity(when):
        chain()
        ctx.sync()
        assert np.array_equal(d_sums.download(np.uint64, span), want_sums), "Q18 sums parity (%s)" % when
        got = np.unpackbits(bm_o.download(np.uint64, ow).view(np.uint8), bitorder="little")[:n_orders].astype(bool)
        assert np.array_equal(got, large), "Q18 orders parity (%s)" % when
        sums(skey, sqty, None, d_sums2)
        ship.lay.scan_group_sum_dense(ship.words, qty.lay, qty.words, day0, days, d_day_sums, None, d_lcnt)
        ctx.sync()
        assert np.array_equal(d_sums2.download(np.uint64, span), want_sums), "shuffled sums parity (%s)" % when
        assert np.array_equal(d_day_sums.download(np.uint64, days), want_days), "ship date sums parity (%s)" % when

    parity("before timing")

    def knob(name, value, fn):
        def run():
            adac.set_tuning(name, value)
            fn()
            adac.set_tuning(name, 1)
        return run

    def by_day(d0, nd):
        return lambda: ship.lay.scan_group_sum_dense(ship.words, qty.lay, qty.words, d0, nd, d_day_sums, None, d_lcnt)

    entries = [("q18_chain", chain),
               ("sum_dense", sums),
               ("sum_dense_no_combine", knob("group_dense_combine", 0, sums)),
               ("sum_dense_with_counts", lambda: sums(counts=d_counts)),
               ("sum_dense_with_counts_no_combine", knob("group_dense_combine", 0, lambda: sums(counts=d_counts))),
               ("count_dense", lambda: lkey.lay.scan_group_count_dense(lkey.words, base, span, d_counts, d_lcnt)),
               ("build_member", lambda: lkey.lay.scan_build_member(lkey.words, base, span, d_set, d_lcnt)),
               ("clear_sums", lambda: d_sums2.zero()),
               ("unpack_keys", lambda: lkey.lay.unpack(lkey.words, d_out)),
               ("unpack_values", lambda: qty.lay.unpack(qty.words, d_out)),
               ("sum_dense_shuffled", lambda: sums(skey, sqty, None, d_sums2)),
               ("sum_dense_shuffled_no_combine", knob("group_dense_combine", 0, lambda: sums(skey, sqty, None, d_sums2))),
               ("shipdate_all_days", by_day(day0, days)),
               ("shipdate_one_year_window", by_day(year0, year)),
               ("shipdate_one_year_direct", knob("group_dense_window", 0, by_day(year0, year)))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    unpack = med["unpack_keys"] + med["unpack_values"]
    kind32 = (4, True)

    def census(k, v, b, nb):
        fs = forms.dense_form_groups(k.descs, kind32, b, nb, v.descs, kind32)
        return {f: fs.count(f) for f in sorted(set(fs) - {None})}

    def cell(call):
        return {"ms": med[call], "over_unpack_of_both": med[call] / unpack, "over_build_member": med[call] / med["build_member"],
                "rows_per_ns": n / (med[call] * 1e6)}

    out = {"orders": n_orders, "lineitems": n, "key_span": span, "sums_bytes": span * 8,
           "orders_over_%d" % Q18_QUANTITY: int(large.sum()),
           "widths": {"l_orderkey": lkey.widths, "l_quantity": qty.widths, "l_orderkey_shuffled": skey.widths,
                      "l_shipdate": ship.widths, "o_orderkey": okey.widths},
           "packed_bytes": {"l_orderkey": lkey.nbytes, "l_quantity": qty.nbytes, "l_shipdate": ship.nbytes},
           "segments_by_form": {"l_orderkey": census(lkey, qty, base, span), "shuffled": census(skey, sqty, base, span),
                                "shipdate_all_days": census(ship, qty, day0, days),
                                "shipdate_one_year": census(ship, qty, year0, year)},
           "ms": med, "q18_chain_ms": med["q18_chain"], "unpack_of_both_ms": unpack,
           "sum_dense": cell("sum_dense"), "sum_dense_no_combine": cell("sum_dense_no_combine"),
           "sum_dense_with_counts": cell("sum_dense_with_counts"), "count_dense": cell("count_dense"),
           "sum_dense_shuffled": cell("sum_dense_shuffled"), "shipdate_all_days": cell("shipdate_all_days"),
           "combine_gain_sorted": med["sum_dense_no_combine"] / med["sum_dense"],
           "combine_gain_shuffled": med["sum_dense_shuffled_no_combine"] / med["sum_dense_shuffled"],
           "window_gain_one_year": med["shipdate_one_year_direct"] / med["shipdate_one_year_window"],
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()},
           "note": ("Synthetic orders / lineitem at SF10 size.  Every sum_dense* call includes clearing its key_span-word "
                    "outputs (clear_sums = one such clear alone).  *_no_combine = group_dense_combine 0 (one atomic per "
                    "row), shipdate_one_year_direct = group_dense_window 0; build_member = adac_scan_build_member over "
                    "l_orderkey and the same domain; unpack_* = adac_unpack of the column.  "
                    "Medians of %d interleaved rounds of %d calls each" % (ROUNDS, INNER))}
    print("q18_packed chain %.4f ms; sum %.4f (no combine %.4f, with counts %.4f, count %.4f, shuffled %.4f); "
          "build_member %.4f, unpack of both %.4f; ship date %.4f, one year window %.4f / direct %.4f"
          % (med["q18_chain"], med["sum_dense"], med["sum_dense_no_combine"], med["sum_dense_with_counts"],
             med["count_dense"], med["sum_dense_shuffled"], med["build_member"], unpack, med["shipdate_all_days"],
             med["shipdate_one_year_window"], med["shipdate_one_year_direct"]), file=sys.stderr, flush=True)
    ctx.close()
    return out


Q5_SUPPLIERS, Q5_NATIONS = 100_000, 25
Q5_REGION = (8, 9, 12, 18, 21)        # the nations of one region (ASIA)
Q5_DATES = (8766, 9130)               # o_orderdate in 1994


def q5_packed(adac, n=59_986_052, n_orders=15_000_000):
    """TPC-H Q5's aggregate on packed columns: SUM(l_extendedprice), COUNT(*) GROUP BY the nation of the supplier behind
    l_suppkey, as adac_scan_group_sum_mapped through a 100 000-byte supplier -> nation map, checked against numpy before
    and after the timing.  Synthetic tables at SF10 size: 60 M lineitems, l_suppkey uniform in 1 .. 100 000,
    l_extendedprice; a map of 25 nation codes, and a second map where the suppliers outside five nations carry 255 (the
    region filter: four rows in five leave through the overflow entry).  Interleaved in the same process: the sum with
    and without d_counts, the count entry, both maps, group_mapped_copies 0 and 1; the sorted-key case, l_orderkey as in
    q18_packed against a 60 M-byte order -> nation map that adac_scan_build_map builds from the orders table under a date
    bitmap (that build timed on its own), on the rows as they are and shuffled; and the comparison points, never the code
    under test: adac_unpack of the two columns, adac_scan_group_sum_dense over the same keys (what a caller had to use
    before; its host-side fold through the map is not timed, which favours it) and adac_scan_group_sum_valid over a
    pre-materialised uint8 code column (the same bins without a look-up: the floor)."""
    ctx = adac.Context(0)
    rng = np.random.default_rng(1995)
    ng = Q5_NATIONS
    cols = lineitem(rng, n, ("l_extendedprice",))
    l_suppkey = rng.integers(1, Q5_SUPPLIERS + 1, size=n).astype(np.int32)
    s_nation = rng.integers(0, ng, size=Q5_SUPPLIERS).astype(np.uint8)
    s_region = np.where(np.isin(s_nation, Q5_REGION), s_nation, 255).astype(np.uint8)
    lc = adac.appender_segment_counts(n, 4)
    price, supp = encode_column(adac, ctx, cols["l_extendedprice"], lc), encode_column(adac, ctx, l_suppkey, lc)
    code_all = encode_column(adac, ctx, s_nation[l_suppkey - 1], lc)   # the pre-materialised code columns
    code_reg = encode_column(adac, ctx, s_region[l_suppkey - 1], lc)
    # the sorted-key case: orders and their lineitems as in q18_packed, the nation of the order's customer per order
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)
    del idx
    l_orderkey = np.repeat(o_orderkey, rng.integers(1, 8, size=n_orders))
    no = len(l_orderkey)
    o_nation = rng.integers(0, ng, size=n_orders).astype(np.uint8)
    o_orderdate = rng.integers(8036, 10562, size=n_orders).astype(np.int32)
    o_price = LINEITEM["l_extendedprice"](rng, no)
    perm = rng.permutation(no)
    oc, olc = adac.appender_segment_counts(n_orders, 4), adac.appender_segment_counts(no, 4)
    okey, onat = encode_column(adac, ctx, o_orderkey, oc), encode_column(adac, ctx, o_nation, oc)
    odate = encode_column(adac, ctx, o_orderdate, oc)
    lkey, lprice = encode_column(adac, ctx, l_orderkey, olc), encode_column(adac, ctx, o_price, olc)
    skey, sprice = encode_column(adac, ctx, l_orderkey[perm], olc), encode_column(adac, ctx, o_price[perm], olc)
    obase, ospan = 1, int(o_orderkey.max())

    def map_buffer(codes):
        buf = np.full((len(codes) + 7) // 8 * 8, 255, dtype=np.uint8)
        buf[:len(codes)] = codes
        return ctx.upload(buf)

    d_map_all, d_map_reg = map_buffer(s_nation), map_buffer(s_region)
    d_omap = ctx.alloc((ospan + 7) // 8 * 8)
    ow, lseg, oseg, olseg = (n_orders + 63) // 64, len(lc), len(oc), len(olc)
    bm_o, d_ocnt = ctx.alloc(ow * 8 + 8), ctx.alloc(oseg * 8)
    d_s, d_c, d_s2, d_c2 = (ctx.alloc((ng + 1) * 8) for _ in range(4))
    d_dense_s, d_dense_c = ctx.alloc(max(Q5_SUPPLIERS, ospan) * 8), ctx.alloc(Q5_SUPPLIERS * 8)
    d_rows = ctx.alloc(max(lseg, olseg, oseg) * 8)
    d_out = ctx.alloc(max(n, no) * 4 + 64)

    def mapped(d_map=d_map_all, counts=None, s=d_s):
        supp.lay.scan_group_sum_mapped(supp.words, price.lay, price.words, d_map, 1, Q5_SUPPLIERS, ng, s, counts, d_rows)

    def count_mapped(d_map=d_map_all):
        supp.lay.scan_group_count_mapped(supp.words, d_map, 1, Q5_SUPPLIERS, ng, d_c, d_rows)

    def order_select():
        odate.lay.scan_select_between(odate.words, Q5_DATES[0], Q5_DATES[1], bm_o, d_ocnt)

    def order_build():
        okey.lay.scan_build_map(okey.words, onat.lay, onat.words, obase, ospan, d_omap, 255, d_rows, bm_o)

    def order_mapped(k=lkey, v=lprice, s=d_s2, c=d_c2):
        k.lay.scan_group_sum_mapped(k.words, v.lay, v.words, d_omap, obase, ospan, ng, s, c, d_rows)

    def fold(codes, keys, values):
        g = np.minimum(codes.astype(np.int64), ng)[keys]
        return (np.bincount(g, weights=values.astype(np.float64), minlength=ng + 1).astype(np.uint64),
                np.bincount(g, minlength=ng + 1).astype(np.uint64))

    # (sums below 2^53: 60 M rows of at most 10 495 000 add up to 6.3e14, exact in the float64 weights of bincount)
    want_all, want_reg = (fold(m, l_suppkey - 1, cols["l_extendedprice"]) for m in (s_nation, s_region))
    year = (o_orderdate >= Q5_DATES[0]) & (o_orderdate <= Q5_DATES[1])
    omap = np.full(ospan, 255, dtype=np.uint8)
    omap[(o_orderkey[year] - obase).astype(np.int64)] = o_nation[year]
    want_ord = fold(omap, (l_orderkey - obase).astype(np.int64), o_price)

    def outputs(s, c):
        return s.download(np.uint64, ng + 1), c.download(np.uint64, ng + 1)

    def parity(when):
        for d_map, want, name in ((d_map_all, want_all, "nations"), (d_map_reg, want_reg, "region")):
            for copies in (0, 1):
                adac.set_tuning("group_mapped_copies", copies)
                mapped(d_map, d_c)
                count_mapped(d_map)
                adac.set_tuning("group_mapped_copies", 0)
                ctx.sync()
                got = outputs(d_s, d_c)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), \
                    "Q5 %s parity, copies %d (%s)" % (name, copies, when)
        order_select()
        order_build()
        ctx.sync()
        assert np.array_equal(d_omap.download(np.uint8, ospan), omap), "order map parity (%s)" % when
        for k, v, name in ((lkey, lprice, "sorted"), (skey, sprice, "shuffled")):
            order_mapped(k, v)
            ctx.sync()
            got = outputs(d_s2, d_c2)
            assert np.array_equal(got[0], want_ord[0]) and np.array_equal(got[1], want_ord[1]), \
                "Q5 through the orders, %s (%s)" % (name, when)

    parity("before timing")

    def one_copy(fn):
        def run():
            adac.set_tuning("group_mapped_copies", 1)
            fn()
            adac.set_tuning("group_mapped_copies", 0)
        return run

    def dense(k, v, b, nb):
        return lambda: k.lay.scan_group_sum_dense(k.words, v.lay, v.words, b, nb, d_dense_s, None, d_rows)

    def valid(v, k):
        return lambda: v.lay.scan_group_sum_valid(v.words, k.lay, k.words, None, ng, d_s2, d_c2)

    entries = [("sum_mapped", mapped),
               ("sum_mapped_with_counts", lambda: mapped(counts=d_c)),
               ("count_mapped", count_mapped),
               ("sum_mapped_region", lambda: mapped(d_map_reg)),
               ("sum_mapped_region_with_counts", lambda: mapped(d_map_reg, d_c)),
               ("count_mapped_region", lambda: count_mapped(d_map_reg)),
               ("sum_mapped_one_copy", one_copy(mapped)),
               ("sum_mapped_region_one_copy", one_copy(lambda: mapped(d_map_reg))),
               ("unpack_suppkey", lambda: supp.lay.unpack(supp.words, d_out)),
               ("unpack_price", lambda: price.lay.unpack(price.words, d_out)),
               ("sum_dense_suppkey", dense(supp, price, 1, Q5_SUPPLIERS)),
               ("sum_valid_codes", valid(price, code_all)),
               ("sum_valid_codes_region", valid(price, code_reg)),
               ("orders_select_dates", order_select),
               ("orders_build_map", order_build),
               ("sum_mapped_orderkey", order_mapped),
               ("sum_mapped_orderkey_shuffled", lambda: order_mapped(skey, sprice)),
               ("unpack_orderkey", lambda: lkey.lay.unpack(lkey.words, d_out)),
               ("unpack_order_price", lambda: lprice.lay.unpack(lprice.words, d_out)),
               ("sum_dense_orderkey", dense(lkey, lprice, obase, ospan)),
               ("sum_dense_orderkey_shuffled", dense(skey, sprice, obase, ospan))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    unpack_supp = med["unpack_suppkey"] + med["unpack_price"]
    unpack_ord = med["unpack_orderkey"] + med["unpack_order_price"]
    kind32 = (4, True)

    def census(k, v, b, nb):
        fs = forms.mapped_form_groups(k.descs, kind32, b, nb, v.descs, kind32)
        return {f: fs.count(f) for f in sorted(set(fs) - {None})}

    def cell(call, rows, unpack, dense_call, floor=None):
        c = {"ms": med[call], "rows_per_ns": rows / (med[call] * 1e6), "over_unpack_of_both": med[call] / unpack,
             "over_sum_dense": med[call] / med[dense_call]}
        if floor:
            c["over_sum_valid_on_codes"] = med[call] / med[floor]
        return c

    s5 = ("sum_dense_suppkey",)
    out = {"lineitems": n, "suppliers": Q5_SUPPLIERS, "nations": ng, "orders": n_orders, "order_lineitems": no,
           "order_key_span": ospan, "orders_in_dates": int(year.sum()),
           "rows_kept_by_region": int(want_reg[1][:ng].sum()),
           "widths": {"l_suppkey": supp.widths, "l_extendedprice": price.widths, "l_orderkey": lkey.widths,
                      "l_orderkey_shuffled": skey.widths, "o_orderkey": okey.widths},
           "packed_bytes": {"l_suppkey": supp.nbytes, "l_extendedprice": price.nbytes, "l_orderkey": lkey.nbytes},
           "segments_by_form": {"l_suppkey": census(supp, price, 1, Q5_SUPPLIERS),
                                "l_orderkey": census(lkey, lprice, obase, ospan),
                                "l_orderkey_shuffled": census(skey, sprice, obase, ospan)},
           "ms": med, "unpack_of_both_ms": {"l_suppkey": unpack_supp, "l_orderkey": unpack_ord},
           "sum_mapped": cell("sum_mapped", n, unpack_supp, *s5, "sum_valid_codes"),
           "sum_mapped_with_counts": cell("sum_mapped_with_counts", n, unpack_supp, *s5, "sum_valid_codes"),
           "count_mapped": cell("count_mapped", n, unpack_supp, *s5),
           "sum_mapped_region": cell("sum_mapped_region", n, unpack_supp, *s5, "sum_valid_codes_region"),
           "sum_mapped_region_with_counts": cell("sum_mapped_region_with_counts", n, unpack_supp, *s5,
                                                 "sum_valid_codes_region"),
           "sum_mapped_orderkey": cell("sum_mapped_orderkey", no, unpack_ord, "sum_dense_orderkey"),
           "sum_mapped_orderkey_shuffled": cell("sum_mapped_orderkey_shuffled", no, unpack_ord,
                                                "sum_dense_orderkey_shuffled"),
           "copies_gain": med["sum_mapped_one_copy"] / med["sum_mapped"],
           "copies_gain_region": med["sum_mapped_region_one_copy"] / med["sum_mapped_region"],
           "orders_build_map_ms": med["orders_build_map"],
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()},
           "note": ("Synthetic lineitem / orders at SF10 size.  sum_dense_* = adac_scan_group_sum_dense over the same keys "
                    "(its host-side fold through the map is not timed); sum_valid_codes* = adac_scan_group_sum_valid over a "
                    "pre-materialised uint8 code column; *_one_copy = group_mapped_copies 1; unpack_* = adac_unpack of the "
                    "column; orders_build_map = adac_scan_build_map over o_orderkey / the nation codes under the date "
                    "bitmap, its %d-byte fill included.  "
                    "Medians of %d interleaved rounds of %d calls each" % ((ospan + 7) // 8 * 8, ROUNDS, INNER))}
    print("q5_packed sum_mapped %.4f ms (with counts %.4f, count %.4f; region %.4f; one copy %.4f / %.4f); unpack of both "
          "%.4f, sum_dense %.4f, sum_valid on codes %.4f / %.4f; through the orders %.4f (shuffled %.4f), unpack %.4f, "
          "sum_dense %.4f (shuffled %.4f); build_map %.4f"
          % (med["sum_mapped"], med["sum_mapped_with_counts"], med["count_mapped"], med["sum_mapped_region"],
             med["sum_mapped_one_copy"], med["sum_mapped_region_one_copy"], unpack_supp, med["sum_dense_suppkey"],
             med["sum_valid_codes"], med["sum_valid_codes_region"], med["sum_mapped_orderkey"],
             med["sum_mapped_orderkey_shuffled"], unpack_ord, med["sum_dense_orderkey"],
             med["sum_dense_orderkey_shuffled"], med["orders_build_map"]), file=sys.stderr, flush=True)
    ctx.close()
    return out


def q5_revenue_packed(adac, n=59_986_052, n_orders=15_000_000, profile=None):
    """TPC-H Q5's revenue on packed columns: SUM(l_extendedprice * l_discount), SUM(l_extendedprice), COUNT(*) GROUP BY the
    nation of the supplier behind l_suppkey from ONE adac_scan_group_sum_product_mapped, so that revenue =
    100 * sums_a - sums_ab = SUM(price * (100 - discount)); checked against numpy before and after the timing.
    q5_packed's tables plus l_discount: 60 M lineitems through the 100 000-byte supplier -> nation map with and without
    the region filter, and the sorted and the shuffled l_orderkey through the 60 M-byte order -> nation map that
    adac_scan_build_map builds under the date bitmap.  Interleaved in the same process: the call with every output and
    with d_sums_a and d_counts NULL, and the comparison points, never the code under test: adac_unpack of the three
    columns, adac_scan_group_sum_mapped on the price alone (the same scan minus b and the product: a floor) and
    adac_scan_group_sum_product over a pre-materialised uint8 code column (the same arithmetic minus the look-up).  The
    results go to profiles/r17_group_product_mapped.json (`profile`: another path) as well as to the caller."""
    ctx = adac.Context(0)
    rng = np.random.default_rng(1997)
    ng = Q5_NATIONS
    cols = lineitem(rng, n, ("l_extendedprice", "l_discount"))
    l_suppkey = rng.integers(1, Q5_SUPPLIERS + 1, size=n).astype(np.int32)
    s_nation = rng.integers(0, ng, size=Q5_SUPPLIERS).astype(np.uint8)
    s_region = np.where(np.isin(s_nation, Q5_REGION), s_nation, 255).astype(np.uint8)
    lc = adac.appender_segment_counts(n, 4)
    price, disc = (encode_column(adac, ctx, cols[c], lc) for c in ("l_extendedprice", "l_discount"))
    supp = encode_column(adac, ctx, l_suppkey, lc)
    code_all = encode_column(adac, ctx, s_nation[l_suppkey - 1], lc)   # the pre-materialised code columns
    code_reg = encode_column(adac, ctx, s_region[l_suppkey - 1], lc)
    # the sorted-key case: orders and their lineitems as in q5_packed
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)
    del idx
    l_orderkey = np.repeat(o_orderkey, rng.integers(1, 8, size=n_orders))
    no = len(l_orderkey)
    o_nation = rng.integers(0, ng, size=n_orders).astype(np.uint8)
    o_orderdate = rng.integers(8036, 10562, size=n_orders).astype(np.int32)
    o_cols = lineitem(rng, no, ("l_extendedprice", "l_discount"))
    perm = rng.permutation(no)
    oc, olc = adac.appender_segment_counts(n_orders, 4), adac.appender_segment_counts(no, 4)
    okey, onat = encode_column(adac, ctx, o_orderkey, oc), encode_column(adac, ctx, o_nation, oc)
    odate = encode_column(adac, ctx, o_orderdate, oc)
    obase, ospan = 1, int(o_orderkey.max())
    year = (o_orderdate >= Q5_DATES[0]) & (o_orderdate <= Q5_DATES[1])
    omap = np.full(ospan, 255, dtype=np.uint8)
    omap[(o_orderkey[year] - obase).astype(np.int64)] = o_nation[year]
    o_code = omap[(l_orderkey - obase).astype(np.int64)]
    Side = namedtuple("Side", "key price disc code")
    sorted_, shuffled = (Side(*(encode_column(adac, ctx, v if sel is None else v[sel], olc)
                                for v in (l_orderkey, o_cols["l_extendedprice"], o_cols["l_discount"], o_code)))
                         for sel in (None, perm))

    def map_buffer(codes):
        buf = np.full((len(codes) + 7) // 8 * 8, 255, dtype=np.uint8)
        buf[:len(codes)] = codes
        return ctx.upload(buf)

    d_map_all, d_map_reg = map_buffer(s_nation), map_buffer(s_region)
    d_omap = ctx.alloc((ospan + 7) // 8 * 8)
    ow, lseg, oseg, olseg = (n_orders + 63) // 64, len(lc), len(oc), len(olc)
    bm_o, d_ocnt = ctx.alloc(ow * 8 + 8), ctx.alloc(oseg * 8)
    d_ab, d_a, d_c, d_s2, d_c2 = (ctx.alloc((ng + 1) * 8) for _ in range(5))
    d_rows = ctx.alloc(max(lseg, olseg, oseg) * 8)
    d_out = ctx.alloc(max(n, no) * 4 + 64)

    def revenue(d_map=d_map_all, every=True):
        supp.lay.scan_group_sum_product_mapped(supp.words, price.lay, price.words, disc.lay, disc.words, d_map, 1,
                                               Q5_SUPPLIERS, ng, d_ab, d_a if every else None, d_c if every else None,
                                               d_rows if every else None)

    def order_revenue(t=sorted_, every=True):
        t.key.lay.scan_group_sum_product_mapped(t.key.words, t.price.lay, t.price.words, t.disc.lay, t.disc.words, d_omap,
                                                obase, ospan, ng, d_ab, d_a if every else None, d_c if every else None,
                                                d_rows if every else None)

    def fold(codes, p, d):
        g = np.minimum(codes.astype(np.int64), ng)
        p = p.astype(np.float64)
        return tuple(np.bincount(g, weights=w, minlength=ng + 1).astype(np.uint64)
                     for w in (p * d.astype(np.float64), p, None))

    # (sums below 2^53: 60 M rows of at most 10 495 000 x 10 add up to 6.3e15, exact in the float64 weights of bincount)
    want_all = fold(s_nation[l_suppkey - 1], cols["l_extendedprice"], cols["l_discount"])
    want_reg = fold(s_region[l_suppkey - 1], cols["l_extendedprice"], cols["l_discount"])
    want_ord = fold(o_code, o_cols["l_extendedprice"], o_cols["l_discount"])

    def outputs():
        return tuple(b.download(np.uint64, ng + 1) for b in (d_ab, d_a, d_c))

    def same(got, want, what):
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), what
        # the query's own form: SUM(price * (100 - discount)) per group
        assert np.array_equal(np.uint64(100) * got[1] - got[0], np.uint64(100) * want[1] - want[0]), what

    def parity(when):
        odate.lay.scan_select_between(odate.words, Q5_DATES[0], Q5_DATES[1], bm_o, d_ocnt)
        okey.lay.scan_build_map(okey.words, onat.lay, onat.words, obase, ospan, d_omap, 255, d_rows, bm_o)
        ctx.sync()
        assert np.array_equal(d_omap.download(np.uint8, ospan), omap), "order map parity (%s)" % when
        for copies in (0, 1):
            adac.set_tuning("group_mapped_copies", copies)
            for run, want, name in ((revenue, want_all, "nations"), (lambda **k: revenue(d_map_reg, **k), want_reg, "region"),
                                    (order_revenue, want_ord, "sorted orders"),
                                    (lambda **k: order_revenue(shuffled, **k), want_ord, "shuffled orders")):
                run()
                ctx.sync()
                same(outputs(), want, "Q5 revenue, %s, copies %d (%s)" % (name, copies, when))
                run(every=False)
                ctx.sync()
                assert np.array_equal(d_ab.download(np.uint64, ng + 1), want[0]), (name, copies, when, "sums_ab alone")
            adac.set_tuning("group_mapped_copies", 0)

    parity("before timing")

    def sum_mapped(k, v, d_map, b, nb):
        return lambda: k.lay.scan_group_sum_mapped(k.words, v.lay, v.words, d_map, b, nb, ng, d_s2, d_c2, d_rows)

    def product_on_codes(a, b, k):
        return lambda: a.lay.scan_group_sum_product(a.words, b.lay, b.words, k.lay, k.words, ng, d_s2, d_c2)

    def unpack(c):
        return lambda: c.lay.unpack(c.words, d_out)

    entries = [("revenue", revenue),
               ("revenue_ab_only", lambda: revenue(every=False)),
               ("revenue_region", lambda: revenue(d_map_reg)),
               ("revenue_region_ab_only", lambda: revenue(d_map_reg, every=False)),
               ("unpack_suppkey", unpack(supp)), ("unpack_price", unpack(price)), ("unpack_discount", unpack(disc)),
               ("sum_mapped_price", sum_mapped(supp, price, d_map_all, 1, Q5_SUPPLIERS)),
               ("sum_mapped_price_region", sum_mapped(supp, price, d_map_reg, 1, Q5_SUPPLIERS)),
               ("product_on_codes", product_on_codes(price, disc, code_all)),
               ("product_on_codes_region", product_on_codes(price, disc, code_reg)),
               ("revenue_orderkey", order_revenue),
               ("revenue_orderkey_ab_only", lambda: order_revenue(every=False)),
               ("revenue_orderkey_shuffled", lambda: order_revenue(shuffled)),
               ("revenue_orderkey_shuffled_ab_only", lambda: order_revenue(shuffled, every=False)),
               ("unpack_orderkey", unpack(sorted_.key)), ("unpack_order_price", unpack(sorted_.price)),
               ("unpack_order_discount", unpack(sorted_.disc)),
               ("sum_mapped_orderkey", sum_mapped(sorted_.key, sorted_.price, d_omap, obase, ospan)),
               ("sum_mapped_orderkey_shuffled", sum_mapped(shuffled.key, shuffled.price, d_omap, obase, ospan)),
               ("product_on_order_codes", product_on_codes(sorted_.price, sorted_.disc, sorted_.code)),
               ("product_on_order_codes_shuffled", product_on_codes(shuffled.price, shuffled.disc, shuffled.code))]
    samples = timed_interleaved(ctx, entries)
    parity("after timing")
    med = {k: float(np.median(x)) for k, x in samples.items()}
    unpack_supp = med["unpack_suppkey"] + med["unpack_price"] + med["unpack_discount"]
    unpack_ord = med["unpack_orderkey"] + med["unpack_order_price"] + med["unpack_order_discount"]
    kind32 = (4, True)

    def census(k, a, b, base, nb):
        fs = forms.mapped_product_form_groups(k.descs, kind32, base, nb, a.descs, kind32, b.descs, kind32)
        return {f: fs.count(f) for f in sorted(set(fs) - {None})}

    def cell(call, rows, unpack3, floor, codes):
        return {"ms": med[call], "rows_per_ns": rows / (med[call] * 1e6), "over_unpack_of_three": med[call] / unpack3,
                "over_sum_mapped_on_price": med[call] / med[floor], "over_sum_product_on_codes": med[call] / med[codes],
                "ab_only_over_every_output": med[call + "_ab_only"] / med[call]}

    out = {"lineitems": n, "suppliers": Q5_SUPPLIERS, "nations": ng, "orders": n_orders, "order_lineitems": no,
           "order_key_span": ospan, "orders_in_dates": int(year.sum()),
           "rows_kept_by_region": int(want_reg[2][:ng].sum()), "rows_kept_by_dates": int(want_ord[2][:ng].sum()),
           "widths": {"l_suppkey": supp.widths, "l_extendedprice": price.widths, "l_discount": disc.widths,
                      "l_orderkey": sorted_.key.widths, "l_orderkey_shuffled": shuffled.key.widths},
           "packed_bytes": {"l_suppkey": supp.nbytes, "l_extendedprice": price.nbytes, "l_discount": disc.nbytes,
                            "l_orderkey": sorted_.key.nbytes},
           "segments_by_form": {"l_suppkey": census(supp, price, disc, 1, Q5_SUPPLIERS),
                                "l_orderkey": census(sorted_.key, sorted_.price, sorted_.disc, obase, ospan),
                                "l_orderkey_shuffled": census(shuffled.key, shuffled.price, shuffled.disc, obase, ospan)},
           "ms": med, "unpack_of_three_ms": {"l_suppkey": unpack_supp, "l_orderkey": unpack_ord},
           "revenue": cell("revenue", n, unpack_supp, "sum_mapped_price", "product_on_codes"),
           "revenue_region": cell("revenue_region", n, unpack_supp, "sum_mapped_price_region", "product_on_codes_region"),
           "revenue_orderkey": cell("revenue_orderkey", no, unpack_ord, "sum_mapped_orderkey", "product_on_order_codes"),
           "revenue_orderkey_shuffled": cell("revenue_orderkey_shuffled", no, unpack_ord, "sum_mapped_orderkey_shuffled",
                                             "product_on_order_codes_shuffled"),
           "samples_ms": {k: [round(t, 5) for t in x] for k, x in samples.items()},
           "note": ("Synthetic lineitem / orders at SF10 size; one run on one MI355X.  revenue* = "
                    "adac_scan_group_sum_product_mapped with d_sums_a, d_counts and d_seg_rows (*_ab_only: all three NULL); "
                    "sum_mapped_* = adac_scan_group_sum_mapped on the price with counts (the same scan minus b and the "
                    "product); product_on_*codes* = adac_scan_group_sum_product over a pre-materialised uint8 code column "
                    "(the same arithmetic minus the look-up); unpack_* = adac_unpack of the column.  "
                    "Medians of %d interleaved rounds of %d calls each" % (ROUNDS, INNER))}
    print("q5_revenue_packed: suppliers %.4f ms (ab only %.4f), region %.4f (%.4f); unpack of three %.4f, sum_mapped on the "
          "price %.4f / %.4f, product on codes %.4f / %.4f; through the orders %.4f (shuffled %.4f), unpack of three %.4f, "
          "sum_mapped %.4f (%.4f), product on codes %.4f (%.4f)"
          % (med["revenue"], med["revenue_ab_only"], med["revenue_region"], med["revenue_region_ab_only"], unpack_supp,
             med["sum_mapped_price"], med["sum_mapped_price_region"], med["product_on_codes"],
             med["product_on_codes_region"], med["revenue_orderkey"], med["revenue_orderkey_shuffled"], unpack_ord,
             med["sum_mapped_orderkey"], med["sum_mapped_orderkey_shuffled"], med["product_on_order_codes"],
             med["product_on_order_codes_shuffled"]), file=sys.stderr, flush=True)
    ctx.close()
    path = profile or os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r17_group_product_mapped.json")
    with open(path, "w") as f:
        json.dump({"q5_revenue_packed": out}, f, indent=1, sort_keys=True)
        f.write("\n")
    return out


def bitpacking_select_gather(adac, n=59_986_052):
    """Filter -> project on DuckDB's own BITPACKING blocks: adac_bp_unpack_selected (values only, then values + ids) of
    l_extendedprice (int32, FOR), the 6-valued uint8 code and a sorted copy of l_partkey (DELTA_FOR) under five bitmaps
    — Q6's final bitmap from the three chained adac_bp_scan_select_between calls, Q1's l_shipdate <= cutoff, uniform
    random 10 % and 50 %, one contiguous 10 % run — each interleaved in the same process with adac_bp_unpack of the
    same column.  The timed calls pass no total_out (they only enqueue); values and ids are checked against numpy
    before and after the timing."""
    from oracle import bitpacking as bp
    ctx = adac.Context(0)
    rng = np.random.default_rng(1994)
    cols = lineitem(rng, n, ("l_shipdate", "l_discount", "l_quantity", "l_extendedprice", "code", "l_partkey"))
    cols["l_partkey_sorted"] = np.sort(cols.pop("l_partkey"))
    enc = {name: bitpacking_blocks(adac, ctx, bp.Compressed(v), v.dtype) for name, v in cols.items()}
    nw = (n + 63) // 64
    bm = [ctx.alloc(nw * 8 + 8) for _ in range(3)]
    d_q1 = ctx.alloc(nw * 8 + 8)
    d_cnt = ctx.alloc(max(e.nseg for e in enc.values()) * 8)
    q6_selects(enc, bm, d_cnt)
    ship = enc["l_shipdate"]
    ship.lay.scan_select_between(ship.words, INT32_MIN_BITS, Q1_CUTOFF_DAY, d_q1, d_cnt)
    ctx.sync()
    run = np.zeros(n, dtype=bool)
    run[n // 3:n // 3 + n // 10] = True
    host_masks = {"q6": q6_mask(cols), "q1": cols["l_shipdate"] <= Q1_CUTOFF_DAY, "uniform_10": rng.random(n) < 0.1,
                  "uniform_50": rng.random(n) < 0.5, "run_10": run}
    d_masks = {"q6": bm[2], "q1": d_q1}

    def bits(mask):
        full = np.zeros(nw * 64, dtype=bool)
        full[:n] = mask
        return np.packbits(full, bitorder="little").view(np.uint64)

    for name in ("q6", "q1"):     # the device's bitmaps are the ones numpy expects
        assert np.array_equal(d_masks[name].download(np.uint64, nw), bits(host_masks[name])), name + " bitmap parity"
    for name in ("uniform_10", "uniform_50", "run_10"):
        d_masks[name] = ctx.upload(bits(host_masks[name]))
    d_out, d_ids, d_dec = ctx.alloc(n * 4 + 64), ctx.alloc(n * 8 + 64), ctx.alloc(n * 4 + 64)
    cells = {}
    for cname in ("l_extendedprice", "code", "l_partkey_sorted"):
        col, v = enc[cname], cols[cname]
        cells[cname] = {}
        for mname, mask in host_masks.items():
            d_mask = d_masks[mname]
            want_v, want_i = v[mask], np.flatnonzero(mask).astype(np.uint64)

            def parity(when):
                d_out.zero(), d_ids.zero()
                total = col.lay.unpack_selected(col.words, d_mask, d_out, d_ids)
                assert total == len(want_v), "%s / %s: total (%s)" % (cname, mname, when)
                assert np.array_equal(d_out.download(v.dtype, total), want_v), "%s / %s: values (%s)" % (cname, mname, when)
                assert np.array_equal(d_ids.download(np.uint64, total), want_i), "%s / %s: ids (%s)" % (cname, mname, when)

            parity("before timing")
            s = timed_interleaved(ctx, [
                ("selected", lambda: col.lay.unpack_selected(col.words, d_mask, d_out, None, False)),
                ("decode", lambda: col.lay.unpack(col.words, d_dec)),
                ("selected_ids", lambda: col.lay.unpack_selected(col.words, d_mask, d_out, d_ids, False))])
            parity("after timing")
            med = {k: float(np.median(x)) for k, x in s.items()}
            sel = len(want_v)
            cells[cname][mname] = {
                "selected_rows": sel, "ms": med["selected"], "ms_with_ids": med["selected_ids"],
                "decode_ms": med["decode"], "over_decode": med["selected"] / med["decode"],
                "with_ids_over_decode": med["selected_ids"] / med["decode"], "packed_bytes": col.nbytes,
                "bytes_written": sel * v.dtype.itemsize, "bytes_written_with_ids": sel * (v.dtype.itemsize + 8),
                "decode_bytes_written": n * v.dtype.itemsize,
                "samples_ms": {k: [round(t, 5) for t in x] for k, x in s.items()}}
            print("bitpacking_select_gather %s / %s: %.4f ms (ids %.4f), decode %.4f" %
                  (cname, mname, med["selected"], med["selected_ids"], med["decode"]), file=sys.stderr, flush=True)
    out = {"rows": n, "columns": {k: enc[k].info for k in cells}, "cells": cells,
           "note": "ms / ms_with_ids = adac_bp_unpack_selected without / with d_out_ids, total_out NULL (enqueue only); "
                   "decode_ms = adac_bp_unpack of the same column; medians of %d interleaved rounds of %d calls each; "
                   "the bitmap words read are rows / 8 bytes on top of packed_bytes" % (ROUNDS, INNER)}
    ctx.close()
    return out


def q1_disc_price_packed(adac, n=59_986_052):
    """Q1's sum_disc_price on packed columns: the columns of q1_filtered_packed that this plan reads (flag code,
    l_extendedprice, l_shipdate; same shapes, a random stream of its own) plus an int32 l_discount in [0, 10].  One
    adac_scan_select_between (l_shipdate <= cutoff) writes the bitmap; under it adac_scan_group_sum_valid(price) and
    adac_scan_group_sum_product(price, disc) give SUM(price * (100 - disc)) = 100 SUM(price) - SUM(price * disc) per
    group, checked against numpy before anything is timed.  Beside the new call, masked and unmasked, in the same
    process: what a caller paid before (adac_unpack of the three columns, after which the multiply and the group-by are
    still to do) and a lower bound for any walk of these columns (the grouped SUM of price + the masked SUM of disc)."""
    ctx = adac.Context(0)
    code, price, shipdate, disc = lineitem(np.random.default_rng(1993), n,
                                           ("code", "l_extendedprice", "l_shipdate", "l_discount")).values()
    cutoff = Q1_CUTOFF_DAY
    counts = adac.appender_segment_counts(n, 4)
    klay, kwords, kbytes, kwidths, kdescs = encode_column(adac, ctx, code, counts)
    dlay, dwords, dbytes, dwidths, _ = encode_column(adac, ctx, shipdate, counts)
    play, pwords, pbytes, pwidths, pdescs = encode_column(adac, ctx, price, counts)
    clay, cwords, cbytes, cwidths, cdescs = encode_column(adac, ctx, disc, counts)
    nw = (n + 63) // 64
    d_filter = ctx.alloc(nw * 8 + 8)
    d_selcnt = ctx.alloc(len(counts) * 8)
    d_seg = ctx.alloc(len(counts) * 8)
    select = lambda: dlay.scan_select_between(dwords, INT32_MIN_BITS, cutoff, d_filter, d_selcnt)
    d_sp, d_cp = ctx.alloc(7 * 8), ctx.alloc(7 * 8)    # SUM(price), COUNT(*)
    d_spd, d_cpd = ctx.alloc(7 * 8), ctx.alloc(7 * 8)  # SUM(price * disc), COUNT(*)
    sum_price = lambda: play.scan_group_sum_valid(pwords, klay, kwords, d_filter, 6, d_sp, d_cp)
    product = lambda: play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, d_spd, None, d_filter)

    def plan():
        select()
        sum_price()
        product()

    keep = shipdate <= cutoff
    bins = [(code == g) & keep for g in range(6)]
    exp = [int((price[b].astype(np.int64) * (100 - disc[b])).sum()) for b in bins]

    def parity(what):
        ctx.sync()
        sp, spd = d_sp.download(np.uint64, 7).tolist(), d_spd.download(np.uint64, 7).tolist()
        assert [100 * sp[g] - spd[g] for g in range(6)] == exp and spd[6] == 0, what
        assert d_cp.download(np.uint64, 7).tolist() == [int(b.sum()) for b in bins] + [0], what

    plan()
    parity("Q1 sum_disc_price parity")
    play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, d_spd, d_cpd, d_filter)   # with counts
    ctx.sync()
    assert d_cpd.download(np.uint64, 7).tolist() == d_cp.download(np.uint64, 7).tolist(), "count parity"
    play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, d_spd, d_cpd)             # NULL mask
    ctx.sync()
    allrows = [code == g for g in range(6)]
    assert d_spd.download(np.uint64, 7).tolist() == [int((price[b].astype(np.int64) * disc[b]).sum()) for b in allrows] + [0]
    assert d_cpd.download(np.uint64, 7).tolist() == [int(b.sum()) for b in allrows] + [0], "unmasked parity"
    # every step is timed warm: 20 back-to-back repetitions after one untimed call.  The new call's working set (packed
    # bytes of three columns + the mask, about 240 MB) can stay in the 256 MB Infinity Cache between repetitions, the
    # unpacks' (the same packed bytes + 540 MB of output) cannot: the comparison favours the new call to that extent
    d_out = ctx.alloc(n * 4 + 64)

    def unpack_three():
        play.unpack(pwords, d_out)
        clay.unpack(cwords, d_out)
        klay.unpack(kwords, d_out)

    def lower_bound():
        sum_price()
        clay.scan_sum(cwords, d_seg, d_filter)

    def staged_only():
        adac.set_tuning("group_product_rw", 0)
        product()
        adac.set_tuning("group_product_rw", 1)

    ms = {}
    for name, fn in (("q1_disc_price_on_packed", plan), ("select", select), ("group_sum_price_masked", sum_price),
                     ("group_sum_product_masked", product),
                     ("group_sum_product_masked_with_counts",
                      lambda: play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, d_spd, d_cpd, d_filter)),
                     ("group_sum_product_unmasked",
                      lambda: play.scan_group_sum_product(pwords, clay, cwords, klay, kwords, 6, d_spd)),
                     ("group_sum_product_masked_staged_kernel_only", staged_only),
                     ("unpack_price_discount_and_code", unpack_three),
                     ("group_sum_price_plus_masked_sum_disc", lower_bound)):
        ms[name] = timed(ctx, fn)
    plan()  # leave the plan's results behind and check them once more after the timed loops
    parity("Q1 sum_disc_price parity (after timing)")
    three = pbytes + cbytes + kbytes
    out = {"rows": n, "groups": 6, "cutoff_day": cutoff, "selected_rows": int(keep.sum()),
           "widths": {"l_extendedprice": pwidths, "l_discount": cwidths, "code": kwidths, "l_shipdate": dwidths},
           "packed_bytes": {"l_extendedprice": pbytes, "l_discount": cbytes, "code": kbytes, "l_shipdate": dbytes},
           "step_ms": ms,
           "group_sum_product_packed_read_GBps": (three + n / 8) / (ms["group_sum_product_masked"] * 1e-3) / 1e9,
           "unpack_three_columns_total_GBps": (three + n * (4 + 4 + 1)) / (ms["unpack_price_discount_and_code"] * 1e-3) / 1e9,
           "product_faster_than_unpack": ms["group_sum_product_masked"] < ms["unpack_price_discount_and_code"],
           "masked_over_lower_bound": ms["group_sum_product_masked"] / ms["group_sum_price_plus_masked_sum_disc"],
           "groups_by_form": group_product_form_groups(pdescs, cdescs, kdescs, 6),
           "note": "group_sum_product_masked = adac_scan_group_sum_product(l_extendedprice, l_discount) GROUP BY the flag "
                   "code under the l_shipdate bitmap, without counts; unpack_price_discount_and_code is what a caller paid "
                   "before it could start to multiply and group; group_sum_price_plus_masked_sum_disc is a lower bound for "
                   "any walk of the three columns; all steps warm (20 back-to-back repetitions): the scans' working set of "
                   "about 240 MB fits the 256 MB Infinity Cache, the unpacks' does not"}
    ctx.close()
    return out


def q1_full_packed(adac, n=59_986_052):
    """All of Q1 on packed columns: q1_disc_price_packed's columns (same shapes, a random stream of its own) plus
    l_quantity (1 .. 50) and an int32 l_tax in [0, 8].  One adac_scan_select_between (l_shipdate <= cutoff) writes the
    bitmap; under it three adac_scan_group_sum_valid (quantity, price, discount), two adac_scan_group_sum_product
    ((price, disc), (price, tax)) and one adac_scan_group_sum_product3 (price, disc, tax); q1_outputs makes the eight
    output columns of them.  Every output column is checked against numpy over the kept rows
    before anything is timed.  Timed: every step and the whole plan, warm and INTERLEAVED (one repetition of every step
    per round, so no step has the clock or the cache state of a run of its own), the new call masked / unmasked / with
    its knob at 0, and what a caller paid before: adac_unpack of the four columns the new call reads."""
    ctx = adac.Context(0)
    t = q1_setup(adac, ctx, n)
    enc, res, sum_pdt = t.enc, t.res, t.sum_pdt
    play = enc["l_extendedprice"].lay
    steps = (t.select,) + tuple(fn for _, fn in t.six)

    def plan():
        for f in steps:
            f()

    exp = q1_expected(t.cols, t.kept_bins)

    def outputs():
        ctx.sync()
        return q1_outputs({k: v[0].download(np.uint64, 7).tolist() for k, v in res.items()},
                          {k: res[k][1].download(np.uint64, 7).tolist() for k in ("q", "p", "d")})

    def parity(what):
        got = outputs()
        for name, want in exp.items():
            assert got[name] == want, (what, name)

    plan()
    parity("Q1 parity")
    form_groups = group_product3_form_groups(enc["l_extendedprice"].descs, enc["l_discount"].descs, enc["l_tax"].descs,
                                             enc["code"].descs, 6)
    p64, d64, t64 = (t.cols[k].astype(np.int64) for k in ("l_extendedprice", "l_discount", "l_tax"))
    exp_pdt = [int((p64[b] * d64[b] * t64[b]).sum()) for b in t.kept_bins] + [0]
    for knob in (0, 1):  # both forms; with counts; the hand-over against the mirror
        adac.set_tuning("group_product3_rw", knob)
        sum_pdt(with_counts=True)
        ctx.sync()
        assert res["pdt"][0].download(np.uint64, 7).tolist() == exp_pdt, ("SUM(p d t)", knob)
        assert res["pdt"][1].download(np.uint64, 7).tolist() == exp["count_order"] + [0], ("COUNT", knob)
        assert play.debug_group_handover() == (form_groups["generic"] if knob else 0), ("hand-over", knob)
    sum_pdt(mask=False, with_counts=True)
    ctx.sync()
    assert res["pdt"][0].download(np.uint64, 7).tolist() == [int((p64[b] * d64[b] * t64[b]).sum()) for b in t.all_bins] + [0]
    assert res["pdt"][1].download(np.uint64, 7).tolist() == [int(b.sum()) for b in t.all_bins] + [0], "unmasked parity"
    d_out = ctx.alloc(n * 4 + 64)
    read = ("l_extendedprice", "l_discount", "l_tax", "code")    # what the new call reads

    def unpack_four():
        for k in read:
            enc[k].lay.unpack(enc[k].words, d_out)

    def staged_only():
        adac.set_tuning("group_product3_rw", 0)
        sum_pdt()
        adac.set_tuning("group_product3_rw", 1)

    entries = (("q1_full_on_packed", plan), ("select", t.select)) + t.six + (
        ("group_sum_product3_masked_with_counts", lambda: sum_pdt(with_counts=True)),
        ("group_sum_product3_unmasked", lambda: sum_pdt(mask=False)),
        ("group_sum_product3_masked_staged_kernel_only", staged_only),
        ("unpack_price_discount_tax_and_code", unpack_four))
    # the scans' working sets (the new call's: packed bytes of four columns + the mask, about 270 MB) are near the 256 MB
    # Infinity Cache, the unpacks' (the same packed bytes + 780 MB of output) are far above it
    samples = timed_interleaved(ctx, entries)
    ms = {name: float(np.median(v)) for name, v in samples.items()}
    plan()  # leave the plan's results behind and check them once more after the timed loops
    parity("Q1 parity (after timing)")
    four = sum(enc[k].nbytes for k in read)
    out = {"rows": n, "groups": 6, "cutoff_day": Q1_CUTOFF_DAY, "selected_rows": int(t.keep.sum()),
           "widths": {k: e.widths for k, e in enc.items()}, "packed_bytes": {k: e.nbytes for k, e in enc.items()},
           "rounds": ROUNDS, "calls_per_round": INNER, "step_ms": ms,
           "step_ms_min": {name: float(min(v)) for name, v in samples.items()},
           "sum_of_steps_ms": sum(ms[name] for name, _ in entries[1:8]),
           "group_sum_product3_packed_read_GBps": (four + n / 8) / (ms["group_sum_product3_masked"] * 1e-3) / 1e9,
           "unpack_four_columns_total_GBps": (four + n * (4 + 4 + 4 + 1)) / (ms["unpack_price_discount_tax_and_code"] * 1e-3) / 1e9,
           "product3_faster_than_unpack": ms["group_sum_product3_masked"] < ms["unpack_price_discount_tax_and_code"],
           "product3_over_product": ms["group_sum_product3_masked"] / ms["group_sum_product_price_disc_masked"],
           "register_walk_faster_than_staged_only": ms["group_sum_product3_masked"] < ms["group_sum_product3_masked_staged_kernel_only"],
           "groups_by_form": form_groups,
           "q1_output": q1_json(outputs()),
           "note": "group_sum_product3_masked = adac_scan_group_sum_product3(l_extendedprice, l_discount, l_tax) GROUP BY "
                   "the flag code under the l_shipdate bitmap, without counts; unpack_price_discount_tax_and_code is what a "
                   "caller paid before it could start to multiply and group; q1_full_on_packed = the select + three "
                   "grouped SUMs + two grouped products + the triple product, seven calls; all figures are medians over 8 "
                   "interleaved rounds of the time per call, 5 calls back to back per entry and round, warm, one process "
                   "(step_ms_min: the fastest round)"}
    ctx.close()
    return out


def q1_fused_packed(adac, n=59_986_052):
    """All of Q1's aggregates from ONE scan: q1_full_packed's data (same generator and seed), the same select, and
    adac_scan_group_sum_q1 (price, discount, tax, quantity GROUP BY the flag code under the l_shipdate bitmap) in place of
    the six grouped calls.  All eight Q1 output columns are built from the one call's seven terms (q1_outputs)
    and checked against numpy before and after timing; the seven terms are also held against the six calls' results.
    Timed warm and INTERLEAVED as in q1_full_packed (one process, medians over rounds): the select, each of the six
    grouped calls, the fused call masked / unmasked / with its knob at 0, and adac_unpack of the five columns it reads."""
    ctx = adac.Context(0)
    t = q1_setup(adac, ctx, n)
    enc, res = t.enc, t.res
    read = ("l_extendedprice", "l_discount", "l_tax", "l_quantity", "code")    # what the fused call reads
    (play, pwords), (clay, cwords), (tlay, twords), (qlay, qwords), (klay, kwords) = (enc[k][:2] for k in read)
    d_q1 = ctx.alloc(7 * 7 * 8)

    def fused(mask=True):
        play.scan_group_sum_q1(pwords, clay, cwords, tlay, twords, qlay, qwords, klay, kwords, 6, d_q1,
                               t.d_filter if mask else None)

    def terms():
        ctx.sync()
        return d_q1.download(np.uint64, 49).reshape(7, 7).tolist()

    def outputs():
        tm = terms()
        cnt = tm[adac.Q1_COUNT]
        return q1_outputs({"q": tm[adac.Q1_SUM_Q], "p": tm[adac.Q1_SUM_A], "d": tm[adac.Q1_SUM_B], "pd": tm[adac.Q1_SUM_AB],
                           "pt": tm[adac.Q1_SUM_AC], "pdt": tm[adac.Q1_SUM_ABC]}, {"q": cnt, "p": cnt, "d": cnt})

    def parity(what, exp):
        got = outputs()
        for name, want in exp.items():
            assert got[name] == want, (what, name)

    exp_masked = q1_expected(t.cols, t.kept_bins)
    exp_all = q1_expected(t.cols, t.all_bins)
    form_groups = group_q1_form_groups(*(enc[k].descs for k in read), 6)
    t.select()
    for _, f in t.six:
        f()
    ctx.sync()
    s6 = {k: v[0].download(np.uint64, 7).tolist() for k, v in res.items()}
    c6 = res["p"][1].download(np.uint64, 7).tolist()
    for knob in (0, 1):  # both forms against numpy and against the six calls; the hand-over against the mirror
        adac.set_tuning("group_q1_rw", knob)
        fused()
        parity(("Q1 parity", knob), exp_masked)
        assert terms() == [c6, s6["q"], s6["p"], s6["d"], s6["pd"], s6["pt"], s6["pdt"]], ("the six calls", knob)
        assert play.debug_group_handover() == (form_groups["generic"] if knob else 0), ("hand-over", knob)
    fused(mask=False)
    parity("Q1 parity, unmasked", exp_all)
    d_out = ctx.alloc(n * 4 + 64)

    def unpack_five():
        for k in read:
            enc[k].lay.unpack(enc[k].words, d_out)

    def staged_only():
        adac.set_tuning("group_q1_rw", 0)
        fused()
        adac.set_tuning("group_q1_rw", 1)

    entries = (("select", t.select),) + t.six + (
        ("group_sum_q1_masked", fused), ("group_sum_q1_unmasked", lambda: fused(mask=False)),
        ("group_sum_q1_masked_staged_kernel_only", staged_only), ("unpack_price_discount_tax_quantity_and_code", unpack_five))
    samples = timed_interleaved(ctx, entries)
    ms = {name: float(np.median(v)) for name, v in samples.items()}
    fused()  # leave the masked result behind and check it once more after the timed loops
    parity("Q1 parity (after timing)", exp_masked)
    five = sum(enc[k].nbytes for k in read)
    six_ms = sum(ms[name] for name, _ in t.six)
    out = {"rows": n, "groups": 6, "cutoff_day": Q1_CUTOFF_DAY, "selected_rows": int(t.keep.sum()),
           "widths": {k: e.widths for k, e in enc.items()}, "packed_bytes": {k: e.nbytes for k, e in enc.items()},
           "rounds": ROUNDS, "calls_per_round": INNER, "step_ms": ms,
           "step_ms_min": {name: float(min(v)) for name, v in samples.items()},
           "six_grouped_calls_ms": six_ms,
           "fused_over_six_calls": ms["group_sum_q1_masked"] / six_ms,
           "fused_faster_than_six_calls": ms["group_sum_q1_masked"] < six_ms,
           "group_sum_q1_packed_read_GBps": (five + n / 8) / (ms["group_sum_q1_masked"] * 1e-3) / 1e9,
           "fused_over_unpack_five_columns": ms["group_sum_q1_masked"] / ms["unpack_price_discount_tax_quantity_and_code"],
           "register_walk_faster_than_staged_only": ms["group_sum_q1_masked"] < ms["group_sum_q1_masked_staged_kernel_only"],
           "groups_by_form": form_groups,
           "q1_output": q1_json(outputs()),
           "note": "group_sum_q1_masked = adac_scan_group_sum_q1(l_extendedprice, l_discount, l_tax, l_quantity) GROUP BY the "
                   "flag code under the l_shipdate bitmap: the seven terms all eight Q1 output columns are made of; "
                   "six_grouped_calls_ms = the sum of the medians of the six grouped calls it replaces; all figures are "
                   "medians over 8 interleaved rounds of the time per call, 5 calls back to back per entry and round, "
                   "warm, one process (step_ms_min: the fastest round)"}
    ctx.close()
    # the condition the fused call exists for: it must beat, in this one interleaved process, the six calls it replaces
    assert out["fused_faster_than_six_calls"], "adac_scan_group_sum_q1 %.4f ms is not below the six grouped calls' %.4f ms: %s" % (
        ms["group_sum_q1_masked"], six_ms, json.dumps(ms))
    return out


def c1_lookups(adac, wl, n=10_000_000, nlookups=10_000):
    """C1 (benchmark/micro/succinct/zipf_distribution.cpp:13-48): t1(i UINTEGER) with i = 0..N-1, compacted, then
    `SELECT i FROM t1 WHERE i == k` for Zipf(N, 1.0) keys (mt19937, seed 42).  Each look-up is one fused
    COUNT(== k) over the packed column: segments whose [min, min + 2^w) cannot hold k are skipped by the kernel
    (one 64-byte record read each), so a look-up costs a launch plus one segment's scan."""
    ctx = adac.Context(0)
    vals = np.arange(n, dtype=np.uint32)
    counts = adac.appender_segment_counts(n, 4)
    lay, d_words, nbytes, _, descs = encode_column(adac, ctx, vals, counts)
    keys = (wl.zipf_column(nlookups, np.uint32, domain=n, skew=1.0, seed=42, threads=1).astype(np.int64) - 1) % n
    d_cnt = ctx.alloc(len(counts) * 8)
    lay.scan_count_eq(d_words, int(keys[0]), d_cnt)
    ctx.sync()
    t0 = time.perf_counter()
    for k in keys:
        lay.scan_count_eq(d_words, int(k), d_cnt)
    ctx.sync()
    wall = time.perf_counter() - t0
    hits = int(d_cnt.download(np.uint64, len(counts)).sum())
    assert hits == 1
    ctx.timer_start()
    for k in keys[:2000]:
        lay.scan_count_eq(d_words, int(k), d_cnt)
    dev_ms = ctx.timer_stop() / 2000
    out = {"rows": n, "segments": int(len(counts)), "max_width": int(descs["width"].max()),
           "packed_bytes": nbytes,
           "lookups": nlookups, "lookups_per_s_wall": nlookups / wall, "device_us_per_lookup": dev_ms * 1e3,
           "note": "one fused COUNT(== k) launch per look-up, results stay on the device; wall = Python loop included"}
    ctx.close()
    return out


def main():
    adac = importlib.import_module(PKG)
    adac.build()
    host = importlib.import_module(PKG + ".host")
    lay = importlib.import_module(PKG + ".layout")
    wl = importlib.import_module(PKG + ".workload")
    only = sys.argv[1:]
    jobs = {"plugin_scan": lambda: plugin_scan(host, lay), "adaptive": lambda: adaptive(host, wl),
            "bitpacking_scan": lambda: bitpacking_scan(adac), "q6_packed": lambda: q6_packed(adac),
            "bitpacking_fused_scans": lambda: bitpacking_fused_scans(adac),
            "q6_bitpacking": lambda: q6_bitpacking(adac),
            "q12_bitpacking": lambda: q12_bitpacking(adac),
            "q12_packed": lambda: q12_packed(adac),
            "q4_packed": lambda: q4_packed(adac),
            "q18_packed": lambda: q18_packed(adac),
            "q5_packed": lambda: q5_packed(adac),
            "q5_revenue_packed": lambda: q5_revenue_packed(adac),
            "bitpacking_select_gather": lambda: bitpacking_select_gather(adac),
            "q6_product_packed": lambda: q6_product_packed(adac), "q1_packed": lambda: q1_packed(adac),
            "q1_filtered_packed": lambda: q1_filtered_packed(adac),
            "q1_disc_price_packed": lambda: q1_disc_price_packed(adac),
            "q1_full_packed": lambda: q1_full_packed(adac),
            "q1_fused_packed": lambda: q1_fused_packed(adac),
            "c1_lookups": lambda: c1_lookups(adac, wl)}
    res = {k: f() for k, f in jobs.items() if not only or k in only}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
