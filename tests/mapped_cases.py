"""The reference and the call wrappers shared by the tests of adac_scan_group_sum_mapped / adac_scan_group_count_mapped /
adac_scan_build_map (test_group_mapped_forms.py on the CPU, test_gpu_group_mapped*.py on the GPU).

Expected values are numpy over the ORIGINAL columns: scan_member_cases.member_index gives every row's index t and whether
its key lies in the domain, the map gives the row's code, np.add.at on uint64 arrays gives the ngroups + 1 sums (each value
widened by its own signedness) and counts mod 2^64.  Every call is made twice into poisoned outputs with one spare word
after each, which must stay poison; the two results must be equal."""
import importlib

import numpy as np

import dense_cases as dc
import scan_member_cases as sm
from dense_cases import _same, _twice, poison
from scan_member_cases import POISON, kind
from scan_compare_cases import seg_counts
from test_gpu_sum_product import widen

forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")
MAPPED_SLICE = forms.MAPPED_SLICE
ALL_FORMS = {"header", "walk-slice", "walk-direct", "staged-slice", "staged-direct"}
NGROUPS = (1, 2, 7, 8, 9, 255, 256)


def map_bytes(span):
    """the map's allocation: key_span rounded up to a multiple of 8 bytes"""
    return (span + 7) // 8 * 8


def padded(codes, pad=0xA5):
    """span codes -> the uint8 allocation, its pad bytes set to `pad`"""
    out = np.full(map_bytes(len(codes)), pad, dtype=np.uint8)
    out[:len(codes)] = codes
    return out


def draw_map(rng, span, ngroups, shape="uniform"):
    """span codes: uniform over the groups and the codes just past them, skewed to one code, or mostly 255"""
    top = min(ngroups + 2, 256)
    codes = rng.integers(0, top, size=span).astype(np.uint8)
    if shape == "skewed":
        codes[rng.random(span) < 0.9] = int(rng.integers(0, ngroups))
    elif shape == "mostly255":
        codes[rng.random(span) < 0.9] = 255
    return codes


def expected(keys, vals, codes, base, span, ngroups, keep=None):
    """(sums, counts, wanted rows inside the domain): ngroups + 1 entries, the last one the codes >= ngroups"""
    t, inside = sm.member_index(keys, base, span)
    if keep is not None:
        inside = inside & keep
    g = np.minimum(codes[t[inside].astype(np.int64)].astype(np.int64), ngroups)
    sums, counts = np.zeros(ngroups + 1, dtype=np.uint64), np.zeros(ngroups + 1, dtype=np.uint64)
    np.add.at(sums, g, widen(vals)[inside])
    np.add.at(counts, g, np.uint64(1))
    return sums, counts, inside


def mapped_forms(klay, base, span, vlay=None):
    if vlay is None:
        return forms.mapped_form_groups(klay.get_descs(), kind(klay.dtype), base, span)
    return forms.mapped_form_groups(klay.get_descs(), kind(klay.dtype), base, span, vlay.get_descs(), kind(vlay.dtype))


def run_sum(ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups, d_validity=None, counts=True, seg_rows=True):
    """adac_scan_group_sum_mapped twice -> (sums, counts or None, rows per segment or None)"""
    nseg, n = len(klay.counts), ngroups + 1
    d_s = ctx.alloc(n * 8 + 8)
    d_c = ctx.alloc(n * 8 + 8) if counts else None
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    out = _twice(lambda: klay.scan_group_sum_mapped(kwords, vlay, vwords, d_map, base, span, ngroups, d_s, d_c, d_r,
                                                    d_validity), [(d_s, n), (d_c, n), (d_r, nseg)])
    for b in (d_s, d_c, d_r):
        if b is not None:
            b.free()
    return out


def run_count(ctx, klay, kwords, d_map, base, span, ngroups, d_validity=None, seg_rows=True):
    """adac_scan_group_count_mapped twice -> (counts, rows per segment or None)"""
    nseg, n = len(klay.counts), ngroups + 1
    d_c = ctx.alloc(n * 8 + 8)
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    out = _twice(lambda: klay.scan_group_count_mapped(kwords, d_map, base, span, ngroups, d_c, d_r, d_validity),
                 [(d_c, n), (d_r, nseg)])
    d_c.free()
    if d_r is not None:
        d_r.free()
    return out


def check_mapped(ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups, keep=None, d_mask=None,
                 what="", every_entry=True, pad=0xA5):
    """the sum entry (with counts and rows per segment) against numpy; with every_entry also the sum entry without its
    optional outputs and the count entry.  codes: span bytes; -> (sums, counts, rows inside)"""
    exp_s, exp_c, inside = expected(keys, vals, codes, base, span, ngroups, keep)
    exp_r = np.array(seg_counts(inside, counts), dtype=np.uint64)
    d_map = ctx.upload(padded(codes, pad))
    s, c, r = run_sum(ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups, d_mask)
    _same(s, exp_s, what, "sums")
    _same(c, exp_c, what, "counts")
    _same(r, exp_r, what, "rows per segment")
    assert int(c.sum()) == int(r.sum())
    if every_entry:
        s, _, _ = run_sum(ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups, d_mask, counts=False,
                          seg_rows=False)
        _same(s, exp_s, what, "sums alone")
        c, r = run_count(ctx, klay, kwords, d_map, base, span, ngroups, d_mask)
        _same(c, exp_c, what, "count entry")
        _same(r, exp_r, what, "count entry, rows per segment")
        c, _ = run_count(ctx, klay, kwords, d_map, base, span, ngroups, d_mask, seg_rows=False)
        _same(c, exp_c, what, "count entry alone")
    d_map.free()
    return exp_s, exp_c, inside


# ---------------------------------------------------------------------------------------------------------------------
# the build
# ---------------------------------------------------------------------------------------------------------------------
def code_numbers(codes):
    """the codes column's values as unsigned numbers of their own width, saturated at 255"""
    u = codes.view(np.dtype("u%d" % codes.dtype.itemsize)).astype(np.uint64)
    return np.minimum(u, np.uint64(255)).astype(np.uint8)


def built_map(keys, codes, base, span, fill, keep=None):
    """(the allocation the build writes, the wanted rows inside the domain, the indices that more than one code claims)"""
    t, inside = sm.member_index(keys, base, span)
    if keep is not None:
        inside = inside & keep
    out = np.full(map_bytes(span), fill, dtype=np.uint8)
    idx, c = t[inside].astype(np.int64), code_numbers(codes)[inside]
    out[idx] = c
    lo, hi = np.full(span, 255, dtype=np.int64), np.full(span, -1, dtype=np.int64)
    np.minimum.at(lo, idx, c.astype(np.int64))
    np.maximum.at(hi, idx, c.astype(np.int64))
    return out, inside, np.nonzero((hi >= 0) & (lo != hi))[0]


def run_build(ctx, klay, kwords, clay, cwords, base, span, fill, d_validity=None, seg_rows=True):
    """adac_scan_build_map twice into a poisoned map with a spare word -> (the allocation's bytes, rows per segment)"""
    nseg, nb = len(klay.counts), map_bytes(span)
    d_m = ctx.alloc(nb + 8)
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    got = []
    for _ in range(2):
        d_m.upload(poison(nb // 8 + 1))
        if d_r is not None:
            d_r.upload(poison(nseg + 1))
        klay.scan_build_map(kwords, clay, cwords, base, span, d_m, fill, d_r, d_validity)
        m = d_m.download(np.uint64, nb // 8 + 1)
        assert int(m[nb // 8]) == POISON, "a word past the map was written"
        r = None
        if d_r is not None:
            r = d_r.download(np.uint64, nseg + 1)
            assert int(r[nseg]) == POISON
            r = r[:nseg].copy()
        got.append((m[:nb // 8].copy().view(np.uint8), r))
    d_m.free()
    if d_r is not None:
        d_r.free()
    return got


def check_build(ctx, keys, codes, klay, kwords, clay, cwords, counts, base, span, fill, keep=None, d_mask=None, what=""):
    """the build against numpy: every byte of the allocation, and the rows per segment; an index that rows with
    different codes share may hold any of them (and need not be the same in the two calls)"""
    exp, inside, loose = built_map(keys, codes, base, span, fill, keep)
    exp_r = np.array(seg_counts(inside, counts), dtype=np.uint64)
    t, _ = sm.member_index(keys, base, span)
    claimed = t[inside].astype(np.int64) * 256 + code_numbers(codes)[inside].astype(np.int64)   # (index, code) pairs
    for m, r in run_build(ctx, klay, kwords, clay, cwords, base, span, fill, d_mask):
        _same(r, exp_r, what, "rows per segment")
        firm = np.ones(len(exp), dtype=bool)
        firm[loose] = False
        _same(m[firm], exp[firm], what, "map")
        assert np.isin(loose * 256 + m[loose].astype(np.int64), claimed).all(), (what, "a code no row of the index has")
    return exp, inside


# ---------------------------------------------------------------------------------------------------------------------
# the key width grid: dense_cases.key_width_grid's geometry with the caps on both sides of MAPPED_SLICE
# ---------------------------------------------------------------------------------------------------------------------
def key_width_grid(dtype):
    """(keys, values, [(base, span)] per segment)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(6100 + 8 * dtype.itemsize + (dtype.kind == "i"))
    ks, vs, doms = [], [], []
    for w in range(1, 8 * dtype.itemsize + 1):
        cap = (MAPPED_SLICE // 2, MAPPED_SLICE + 1, 1 << 16)[w % 3]
        k, base, span, _ = sm.grid_segment(rng, dtype, w, cap)
        ks.append(k)
        vs.append(sm.segment_at_width(rng, np.uint16, sm.ROWS_GRID, 1 + (5 * w) % 16))
        doms.append((base, span))
    return np.concatenate(ks), np.concatenate(vs), doms


# ---------------------------------------------------------------------------------------------------------------------
# the fuzz: dense_cases.fuzz_draw's columns and domain (its knob bit drives group_mapped_copies), then ngroups and the
# map from a generator of their own, so that the dense draws stay what they are
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = 32


def fuzz_draw(seed):
    """-> rng, keys, values, counts, rule, pad, base, span, copies knob, ngroups, codes"""
    rng, keys, vals, counts, rule, pad, base, span, knob = dc.fuzz_draw(seed)
    mrng = np.random.default_rng(7000 + seed)
    ngroups = NGROUPS[int(mrng.integers(0, len(NGROUPS)))] if seed % 4 else int(mrng.integers(1, 257))
    codes = draw_map(mrng, span, ngroups, ("uniform", "skewed", "mostly255")[(seed // 3) % 3])
    return rng, keys, vals, counts, rule, pad, base, span, knob, ngroups, codes
