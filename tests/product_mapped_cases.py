"""The reference and the call wrappers shared by the tests of adac_scan_group_sum_product_mapped
(test_group_product_mapped_forms.py on the CPU, test_gpu_group_product_mapped*.py on the GPU).

Expected values are numpy over the ORIGINAL columns: scan_member_cases.member_index gives every row's index t and whether
its key lies in the domain, the map gives the row's code, np.add.at on uint64 arrays of widen(a) * widen(b) (uint64 array
multiplication wraps) and of widen(a) gives the ngroups + 1 sums, each factor widened by its own signedness.  The
comparison is exact.  Every call is made twice into poisoned outputs with one spare word after each, which must stay
poison; the two results must be equal."""
import importlib

import numpy as np

import mapped_cases as mc
import scan_member_cases as sm
from dense_cases import _same, _twice
from scan_member_cases import kind
from scan_compare_cases import seg_counts
from test_gpu_sum_product import widen

forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")

# every combination of the optional outputs d_sums_a and d_counts
OUTPUTS = ((True, True), (True, False), (False, True), (False, False))


def expected(keys, a, b, codes, base, span, ngroups, keep=None):
    """(sums_ab, sums_a, counts, wanted rows inside the domain): ngroups + 1 entries, the last one the codes >= ngroups"""
    t, inside = sm.member_index(keys, base, span)
    if keep is not None:
        inside = inside & keep
    g = np.minimum(codes[t[inside].astype(np.int64)].astype(np.int64), ngroups)
    sab, sa, cn = (np.zeros(ngroups + 1, dtype=np.uint64) for _ in range(3))
    wa, wb = widen(a)[inside], widen(b)[inside]
    np.add.at(sab, g, wa * wb)
    np.add.at(sa, g, wa)
    np.add.at(cn, g, np.uint64(1))
    return sab, sa, cn, inside


def product_forms(klay, base, span, alay, blay):
    return forms.mapped_product_form_groups(klay.get_descs(), kind(klay.dtype), base, span, alay.get_descs(),
                                            kind(alay.dtype), blay.get_descs(), kind(blay.dtype))


def run_product(ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups, d_validity=None, sums_a=True,
                counts=True, seg_rows=True):
    """adac_scan_group_sum_product_mapped twice -> (sums_ab, sums_a or None, counts or None, rows per segment or None)"""
    nseg, n = len(klay.counts), ngroups + 1
    d_ab = ctx.alloc(n * 8 + 8)
    d_a = ctx.alloc(n * 8 + 8) if sums_a else None
    d_c = ctx.alloc(n * 8 + 8) if counts else None
    d_r = ctx.alloc(nseg * 8 + 8) if seg_rows else None
    out = _twice(lambda: klay.scan_group_sum_product_mapped(kwords, alay, awords, blay, bwords, d_map, base, span, ngroups,
                                                            d_ab, d_a, d_c, d_r, d_validity),
                 [(d_ab, n), (d_a, n), (d_c, n), (d_r, nseg)])
    for buf in (d_ab, d_a, d_c, d_r):
        if buf is not None:
            buf.free()
    return out


def check_product(ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups, keep=None,
                  d_mask=None, what="", every_output=True, pad=0xA5):
    """the call with every output against numpy; with every_output also every combination of d_sums_a / d_counts present
    or NULL (the last one without the rows per segment too).  codes: span bytes; -> (sums_ab, sums_a, counts, inside)"""
    exp_ab, exp_a, exp_c, inside = expected(keys, a, b, codes, base, span, ngroups, keep)
    exp_r = np.array(seg_counts(inside, counts), dtype=np.uint64)
    d_map = ctx.upload(mc.padded(codes, pad))
    for with_a, with_c in (OUTPUTS if every_output else OUTPUTS[:1]):
        rows = with_a or with_c
        sab, sa, c, r = run_product(ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups, d_mask,
                                    sums_a=with_a, counts=with_c, seg_rows=rows)
        tag = (what, "sums_a" if with_a else "-", "counts" if with_c else "-")
        _same(sab, exp_ab, tag, "sums_ab")
        if with_a:
            _same(sa, exp_a, tag, "sums_a")
        if with_c:
            _same(c, exp_c, tag, "counts")
            assert int(c.sum()) == int(exp_r.sum())
        if rows:
            _same(r, exp_r, tag, "rows per segment")
    d_map.free()
    return exp_ab, exp_a, exp_c, inside


def cycled(rng, dtype, rows, widths):
    """one segment of `rows` values per width of `widths`, back to back"""
    return np.concatenate([sm.segment_at_width(rng, dtype, rows, int(w)) for w in widths])


# ---------------------------------------------------------------------------------------------------------------------
# the key width grid: mapped_cases.key_width_grid's keys and domains (its value column is `a`: widths 1 + (5 w) % 16), and
# a second value column whose widths cycle on their own, 1 + (3 w + 7) % 16
# ---------------------------------------------------------------------------------------------------------------------
def key_width_grid(dtype):
    """(keys, a, b, [(base, span)] per segment)"""
    dtype = np.dtype(dtype)
    keys, a, doms = mc.key_width_grid(dtype)
    rng = np.random.default_rng(8100 + 8 * dtype.itemsize + (dtype.kind == "i"))
    b = cycled(rng, np.int16, sm.ROWS_GRID, [1 + (3 * w + 7) % 16 for w in range(1, 8 * dtype.itemsize + 1)])
    return keys, a, b, doms


# ---------------------------------------------------------------------------------------------------------------------
# the value widths: 64 segments x 257 rows, the key at w = 13; one column sweeps the widths 1 ... 64 of an 8-byte type,
# the other one cycles 1 + (7 w) % 32
# ---------------------------------------------------------------------------------------------------------------------
VW_ROWS, VW_SEGS = 257, 64


def value_width_columns(vtype):
    """(keys, the sweeping column, the cycling column of the same type, the widths of the cycling column)"""
    vtype = np.dtype(vtype)
    rng = np.random.default_rng(8200 + (vtype.kind == "i"))
    n = VW_ROWS * VW_SEGS
    keys = (1000 + rng.integers(200, 4000, size=n)).astype(np.uint32)
    keys[rng.random(n) < 0.2] = 1000 + 7000   # outside the domains of the test
    keys[0::VW_ROWS], keys[1::VW_ROWS] = 1000, 1000 + (1 << 13) - 1
    cyc = [1 + (7 * w) % 32 for w in range(1, 65)]
    return keys, cycled(rng, vtype, VW_ROWS, range(1, 65)), cycled(rng, vtype, VW_ROWS, cyc), cyc


# ---------------------------------------------------------------------------------------------------------------------
# the lanes bound: one segment of 24 577 rows (two scan groups, uneven quarters), the key at w = 4, the most rows per
# chunk; and the counts of test_gpu_group_mapped.ngroups_column with the third segment's key at w = 40
# ---------------------------------------------------------------------------------------------------------------------
LANES_WIDTHS = ((32, 5), (5, 32), (32, 32))


def lanes_columns(wa, wb, counts=(24577,), wide_last=False):
    """(keys, a, b, counts): keys at w = 4 (the last segment at w = 40 with wide_last); a (uint64) and b (int64) packed at
    exactly wa and wb bits against a frame"""
    rng = np.random.default_rng(8300 + 40 * wa + wb + len(counts))
    counts = np.array(counts, dtype=np.uint32)
    ks, as_, bs = [], [], []
    for i, c in enumerate(counts):
        c = int(c)
        if wide_last and i == len(counts) - 1:
            k = (rng.integers(0, 1 << 40, size=c, dtype=np.uint64) + np.uint64(700)).astype(np.uint64)
            k[0], k[1] = 700, 700 + (1 << 40) - 1
            k[2::3] = 700 + rng.integers(0, 16, size=len(k[2::3]), dtype=np.uint64)
        else:
            k = (rng.integers(0, 16, size=c, dtype=np.uint64) + np.uint64(700)).astype(np.uint64)
            k[0], k[1] = 700, 715
        ks.append(k)
        as_.append(sm.segment_at_width(rng, np.uint64, c, wa))
        bs.append(sm.segment_at_width(rng, np.int64, c, wb))
    return np.concatenate(ks), np.concatenate(as_), np.concatenate(bs), counts


# ---------------------------------------------------------------------------------------------------------------------
# the fuzz: mapped_cases.fuzz_draw for keys, a, domain, knob, ngroups and map; b from a generator of its own, so that
# the existing draws stay what they are
# ---------------------------------------------------------------------------------------------------------------------
B_TYPES = (np.int8, np.uint8, np.int16, np.uint32, np.int64, np.uint64)


def fuzz_draw(seed):
    """-> rng, keys, a, b, counts, rule, pad, base, span, copies knob, ngroups, codes"""
    rng, keys, a, counts, rule, pad, base, span, knob, ngroups, codes = mc.fuzz_draw(seed)
    brng = np.random.default_rng(9000 + seed)
    bt = np.dtype(B_TYPES[int(brng.integers(0, len(B_TYPES)))])
    segs = [sm.segment_at_width(brng, bt, max(int(c), 2), int(brng.integers(1, 8 * bt.itemsize + 1)))[:int(c)]
            for c in counts]
    return rng, keys, a, np.concatenate(segs), counts, rule, pad, base, span, knob, ngroups, codes
