"""The reference and the call wrappers shared by the tests of adac_scan_group_sum_dense / adac_scan_group_count_dense
(test_group_dense_forms.py on the CPU, test_gpu_group_dense*.py on the GPU).

Expected values are numpy over the ORIGINAL columns: scan_member_cases.member_index gives every row's index t and whether
its key lies in the domain, np.add.at on uint64 arrays gives the sums (each value widened by its own signedness) and the
counts mod 2^64.  Every call is made twice into poisoned outputs with one spare word after each, which must stay
poison; the two results must be equal."""
import importlib

import numpy as np

import scan_member_cases as sm
from scan_member_cases import POISON, kind
from scan_compare_cases import seg_counts
from test_gpu_sum_product import widen

forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")
DENSE_WINDOW = forms.DENSE_WINDOW
ALL_FORMS = {"header", "walk-window", "walk-direct", "staged-window", "staged-direct"}


def expected(keys, vals, base, span, keep=None):
    """(sums, counts, wanted rows inside the domain)"""
    t, inside = sm.member_index(keys, base, span)
    if keep is not None:
        inside = inside & keep
    sums, counts = np.zeros(span, dtype=np.uint64), np.zeros(span, dtype=np.uint64)
    idx = t[inside].astype(np.int64)
    np.add.at(sums, idx, widen(vals)[inside])
    np.add.at(counts, idx, np.uint64(1))
    return sums, counts, inside


def dense_forms(klay, base, span, vlay=None):
    if vlay is None:
        return forms.dense_form_groups(klay.get_descs(), kind(klay.dtype), base, span)
    return forms.dense_form_groups(klay.get_descs(), kind(klay.dtype), base, span, vlay.get_descs(), kind(vlay.dtype))


_poison = {}


def poison(n):
    if n not in _poison:
        _poison[n] = np.full(n, POISON, dtype=np.uint64)
    return _poison[n]


def _twice(call, bufs):
    """bufs: [(device buffer or None, words)] -> the downloaded words of every buffer (None for None)"""
    got = []
    for _ in range(2):
        for b, n in bufs:
            if b is not None:
                b.upload(poison(n + 1))
        call()
        out = []
        for b, n in bufs:
            if b is None:
                out.append(None)
                continue
            w = b.download(np.uint64, n + 1)
            assert int(w[n]) == POISON, "a word past the result was written"
            out.append(w[:n].copy())
        got.append(out)
    for x, y in zip(*got):
        assert (x is None and y is None) or np.array_equal(x, y), "two calls, two results"
    return got[0]


def run_sum(ctx, klay, kwords, vlay, vwords, base, span, d_validity=None, counts=True, seg_rows=True):
    """adac_scan_group_sum_dense twice -> (sums, counts or None, rows per segment or None)"""
    nseg = len(klay.counts)
    d_s = ctx.alloc(span * 8 + 8)
    d_c = ctx.alloc(span * 8 + 8) if counts else None
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    out = _twice(lambda: klay.scan_group_sum_dense(kwords, vlay, vwords, base, span, d_s, d_c, d_r, d_validity),
                 [(d_s, span), (d_c, span), (d_r, nseg)])
    for b in (d_s, d_c, d_r):
        if b is not None:
            b.free()
    return out


def run_count(ctx, klay, kwords, base, span, d_validity=None, seg_rows=True):
    """adac_scan_group_count_dense twice -> (counts, rows per segment or None)"""
    nseg = len(klay.counts)
    d_c = ctx.alloc(span * 8 + 8)
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    out = _twice(lambda: klay.scan_group_count_dense(kwords, base, span, d_c, d_r, d_validity), [(d_c, span), (d_r, nseg)])
    d_c.free()
    if d_r is not None:
        d_r.free()
    return out


def _same(got, exp, what, name):
    wrong = np.nonzero(got != exp)[0]
    assert len(wrong) == 0, (what, name, len(wrong), [(int(i), int(got[i]), int(exp[i])) for i in wrong[:4]])


def check_dense(ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, keep=None, d_mask=None, what="",
                every_entry=True):
    """the sum entry (with counts and rows per segment) against numpy; with every_entry also the sum entry without its
    optional outputs and the count entry"""
    exp_s, exp_c, inside = expected(keys, vals, base, span, keep)
    exp_r = np.array(seg_counts(inside, counts), dtype=np.uint64)
    s, c, r = run_sum(ctx, klay, kwords, vlay, vwords, base, span, d_mask)
    _same(s, exp_s, what, "sums")
    _same(c, exp_c, what, "counts")
    _same(r, exp_r, what, "rows per segment")
    assert int(c.sum()) == int(r.sum())
    if every_entry:
        s, _, _ = run_sum(ctx, klay, kwords, vlay, vwords, base, span, d_mask, counts=False, seg_rows=False)
        _same(s, exp_s, what, "sums alone")
        c, r = run_count(ctx, klay, kwords, base, span, d_mask)
        _same(c, exp_c, what, "count entry")
        _same(r, exp_r, what, "count entry, rows per segment")
        c, _ = run_count(ctx, klay, kwords, base, span, d_mask, seg_rows=False)
        _same(c, exp_c, what, "count entry alone")
    return exp_s, exp_c, inside


def full_mask(keep, counts, offs, span):
    """bool per row -> the u64 words of a mask over the keys' element space (+ a spare word): the elements between the
    segments AND the tail of the last word are set: they belong to no row and must not matter"""
    nw = (max(span, 1) + 63) // 64
    full = np.ones(nw * 64, dtype=bool)
    pos = 0
    for c, o in zip(counts, offs):
        full[int(o):int(o) + int(c)] = keep[pos:pos + int(c)]
        pos += int(c)
    return np.concatenate([np.packbits(full, bitorder="little").view(np.uint64), np.zeros(1, np.uint64)])


# ---------------------------------------------------------------------------------------------------------------------
# the key width grid: scan_member_cases.grid_segment's geometry (the domain strictly inside the interval, rows planted
# below, inside and above), the caps on both sides of DENSE_WINDOW; the value column uint16 at a width per segment
# ---------------------------------------------------------------------------------------------------------------------
def key_width_grid(dtype):
    """(keys, values, [(base, span)] per segment)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(4100 + 8 * dtype.itemsize + (dtype.kind == "i"))
    ks, vs, doms = [], [], []
    for w in range(1, 8 * dtype.itemsize + 1):
        cap = (DENSE_WINDOW // 2, DENSE_WINDOW + 1, 1 << 16)[w % 3]
        k, base, span, _ = sm.grid_segment(rng, dtype, w, cap)
        ks.append(k)
        vs.append(sm.segment_at_width(rng, np.uint16, sm.ROWS_GRID, 1 + (5 * w) % 16))
        doms.append((base, span))
    return np.concatenate(ks), np.concatenate(vs), doms


# ---------------------------------------------------------------------------------------------------------------------
# the fuzz: every seed draws the two types, the segments, the key distribution, the domain, the mask and the knob
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_COUNTS = (0, 1, 63, 64, 65, 257, 1000, 2049, 4097, 9000, 24577)
FUZZ_SEEDS = 32
VALUE_TYPES = (np.int8, np.uint16, np.int32, np.uint64)


def fuzz_draw(seed):
    """-> rng, keys, values, counts, rule, pad, base, span, combine"""
    rng = np.random.default_rng(5000 + seed)
    kt = np.dtype(sm.TYPES[int(rng.integers(0, len(sm.TYPES)))])
    vt = np.dtype(VALUE_TYPES[int(rng.integers(0, len(VALUE_TYPES)))])
    tb = 8 * kt.itemsize
    nseg = int(rng.integers(1, 6))
    counts = np.array([FUZZ_COUNTS[int(rng.integers(0, len(FUZZ_COUNTS)))] for _ in range(nseg)], dtype=np.uint32)
    if not counts.any():
        counts[0] = 257
    shape = ("sorted", "clustered", "uniform")[seed % 3]
    ksegs, vsegs = [], []
    for c in counts:
        c = int(c)
        w = int(rng.integers(1, tb + 1))
        k = sm.segment_at_width(rng, kt, max(c, 2), w)[:c]
        if shape == "sorted":
            k = np.sort(k)
        elif shape == "clustered" and c > 8:   # runs of equal keys, the ends of the interval kept
            k[2:c - 1] = np.repeat(k[2:c - 1:4], 4)[:c - 3]
        ksegs.append(k)
        vsegs.append(sm.segment_at_width(rng, vt, max(c, 2), int(rng.integers(1, 8 * vt.itemsize + 1)))[:c])
    keys, vals = np.concatenate(ksegs), np.concatenate(vsegs)
    rule, pad = int(rng.integers(0, 2)), bool(rng.integers(0, 2))
    # the domain: around a row of the column (so that it meets a segment), or anywhere in the type
    span = min(int(2 ** rng.uniform(0, 18.5)), 1 << tb)
    if rng.random() < 0.8:
        at = int(sm.biased(keys)[int(rng.integers(0, len(keys)))])
        dlo = at - int(rng.integers(0, span))
    else:
        dlo = int(rng.integers(0, (1 << tb) - 1, dtype=np.uint64, endpoint=True))
    dlo = min(max(dlo, 0), (1 << tb) - span)
    return rng, keys, vals, counts, rule, pad, dlo ^ sm.sign_bit(kt), span, int(rng.integers(0, 2))
