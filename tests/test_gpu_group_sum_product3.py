"""adac_scan_group_sum_product3: SUM(a * b * c) GROUP BY key over four packed columns of one table under a selection
bitmap indexed in a's element space (the term Q1's sum_charge adds: 10000 SUM(p) + 100 SUM(p t) - 100 SUM(p d) - SUM(p d t)).

The expected value is numpy over the ORIGINAL columns: each of a, b and c widened to 64 bits by its own signedness and
viewed as uint64, multiplied (uint64 wraps mod 2^64, as the ABI says; tests/test_group_sum_product3_abi.py holds this
product against Python integers), grouped by the key as an unsigned number of its own width (keys >= ngroups in bin
`ngroups`), summed with dtype=uint64.  Compared exactly.  Both kernel forms are held to it: the register walk
(k_group_product3_rw) with the staged kernel (k_group_product3) for what it leaves, and the staged kernel alone under
group_product3_rw = 0.  Results are poisoned before every call and one word past ngroups + 1 is asserted untouched.
Which kernel took what is read back after every call (adac_debug_group_handover) and held against the host mirror of
the eligibility rule (forms.group_product3_form_groups), so the walk cannot quietly hand its work to the staged
kernel."""
import importlib

import numpy as np
import pytest

from test_gpu_group_sum import reference_groups
from test_gpu_group_sum_product import (ALL, COUNTS1, INVALID_ARGUMENT, KEY_CASES, POISON, Col, NullLayout,
                                        column_at_width, mixed_product_column, shared_columns, widen)
from test_gpu_group_sum_product import reference as reference2
from test_gpu_group_sum_rw import every_width_column
from test_gpu_group_sum_valid import clustered, element_mask, make_case, mask_shapes, phase_column

group_product3_form_groups = importlib.import_module("duckdb-adaptive-compression_amd.forms").group_product3_form_groups
pytestmark = pytest.mark.gpu

# (type of b, type of c): every type of {uint8, int16, int32, uint64} once on either side, never twice in a pair
BC_PAIRS = ((np.uint8, np.int16), (np.int16, np.int32), (np.int32, np.uint64), (np.uint64, np.uint8))


class product3_rw:
    """with product3_rw(adac, 0): the staged kernel alone; the default (1) restored on exit."""

    def __init__(self, adac, value):
        self.adac, self.value = adac, value

    def __enter__(self):
        self.adac.set_tuning("group_product3_rw", self.value)

    def __exit__(self, *exc):
        self.adac.set_tuning("group_product3_rw", 1)


def product3(a, b, c):
    """widen(a) * widen(b) * widen(c) as uint64: both multiplications wrap mod 2^64"""
    return widen(a) * widen(b) * widen(c)


def reference(a, b, c, keys, ngroups, keep=None):
    """(sums, counts), ngroups + 1 entries each"""
    p = product3(a, b, c)
    ukeys = keys.view(np.dtype("u%d" % keys.dtype.itemsize)).astype(np.uint64)
    bins = np.minimum(ukeys, np.uint64(ngroups)).astype(np.int64)
    if keep is not None:
        p, bins = p[keep], bins[keep]
    sums = [int(p[bins == g].sum(dtype=np.uint64)) for g in range(ngroups + 1)]
    cnts = np.bincount(bins, minlength=ngroups + 1).tolist()
    return sums, cnts


class Quad:
    def __init__(self, ctx, a, b, c, k, ngroups):
        self.ctx, self.a, self.b, self.c, self.k, self.ngroups = ctx, a, b, c, k, ngroups
        self.span = int(a.lay.value_span)
        self.d_sums, self.d_cnts = ctx.alloc((ngroups + 2) * 8), ctx.alloc((ngroups + 2) * 8)
        self._forms = None

    def forms(self):
        """{"fast": scan groups of a the register walk takes, "generic": the rest} by the host mirror of the rule"""
        if self._forms is None:
            kind = lambda col: (col.vals.dtype.itemsize, col.vals.dtype.kind == "i")
            self._forms = group_product3_form_groups(self.a.lay.get_descs(), self.b.lay.get_descs(),
                                                     self.c.lay.get_descs(), self.k.lay.get_descs(), self.ngroups,
                                                     kind(self.a), kind(self.b), kind(self.c), self.k.vals.dtype.itemsize)
        return self._forms

    def left_to_the_staged_kernel(self, rw=1):
        """what the register walk of a call hands over, by the host mirror: the scan groups it cannot take; nothing when
        it is not launched (knob at 0, more than 8 bins: the staged kernel then takes everything)"""
        return self.forms()["generic"] if rw and self.ngroups + 1 <= 8 else 0

    def call(self, d_mask=None, counts=True, rw=1):
        """-> (sums, counts or None); nothing is written past ngroups + 1 entries; the hand-over word is the mirror's"""
        n = self.ngroups + 1
        self.d_sums.upload(np.full(n + 1, POISON, dtype=np.uint64))
        self.d_cnts.upload(np.full(n + 1, POISON, dtype=np.uint64))
        self.a.lay.scan_group_sum_product3(self.a.words, self.b.lay, self.b.words, self.c.lay, self.c.words, self.k.lay,
                                           self.k.words, self.ngroups, self.d_sums, self.d_cnts if counts else None,
                                           d_mask)
        s, c = self.d_sums.download(np.uint64, n + 1).tolist(), self.d_cnts.download(np.uint64, n + 1).tolist()
        assert s[n] == POISON and c[n] == POISON
        if not counts:
            assert c == [POISON] * (n + 1)
        assert self.a.lay.debug_group_handover() == self.left_to_the_staged_kernel(rw), ("hand-over", rw, self.forms())
        return s[:n], (c[:n] if counts else None)

    def upload_mask(self, keep, outside=False):
        return self.ctx.upload(element_mask(keep, self.a.counts, self.a.offs, self.span, outside))

    def expected(self, keep=None):
        return reference(self.a.vals, self.b.vals, self.c.vals, self.k.vals, self.ngroups, keep)

    def check(self, keep, what, outside=False):
        """One masked call against numpy (keep None: the NULL mask); the counts add up to the kept rows; without
        d_counts the same sums."""
        d_mask = None if keep is None else self.upload_mask(keep, outside)
        exp = self.expected(keep)
        got = self.call(d_mask)
        assert got[0] == exp[0] and got[1] == exp[1], what
        assert sum(got[1]) == (len(self.a.vals) if keep is None else int(keep.sum())), what
        assert self.call(d_mask, counts=False) == (exp[0], None), (what, "no counts")
        if d_mask is not None:
            d_mask.free()
        return got

    def check_three_ways(self, adac, keep, what):
        """The register walk, the staged kernel alone, the register walk again (the hand-over word was left at zero)."""
        d_mask = None if keep is None else self.upload_mask(keep)
        exp = self.expected(keep)
        for rw in (1, 0, 1):
            with product3_rw(adac, rw):
                got = self.call(d_mask, rw=rw)
                assert got[0] == exp[0] and got[1] == exp[1], (what, rw)
                assert self.call(d_mask, counts=False, rw=rw)[0] == exp[0], (what, rw, "no counts")
        if d_mask is not None:
            d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 1. types and masks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adtype", ALL)
def test_every_type_of_a_under_every_mask_shape(adac, gpu_ctx, adtype):
    adtype = np.dtype(adtype)
    cols = shared_columns(adac, gpu_ctx)   # b / c and key columns on COUNTS1, encoded once
    rng = np.random.default_rng(3880 + adtype.itemsize + (adtype.kind == "i"))
    shapes = mask_shapes(np.random.default_rng(11), COUNTS1)
    shapes["NULL"] = None
    tb = 8 * adtype.itemsize
    for vbits in (6, tb // 2 + 1):
        vals, _ = make_case(rng, adtype, np.uint8, int(COUNTS1.sum()), vbits, 2)
        a = Col(adac, gpu_ctx, vals, COUNTS1)
        for bt, ct in BC_PAIRS:
            for kt, ngroups, _ in KEY_CASES:
                q = Quad(gpu_ctx, a, cols["b", np.dtype(bt).name], cols["b", np.dtype(ct).name],
                         cols["k", np.dtype(kt).name], ngroups)
                for name, keep in shapes.items():
                    got = q.check(keep, (vbits, np.dtype(bt).name, np.dtype(ct).name, np.dtype(kt).name, name))
                    if name == "zeros":
                        assert not any(got[0]) and not any(got[1])
                    if name == "ones":
                        assert got[0] == q.expected()[0]


# ---------------------------------------------------------------------------------------------------------------------
# 2. products that wrap
# ---------------------------------------------------------------------------------------------------------------------
def test_products_wrap_mod_2_64(adac, gpu_ctx):
    rng = np.random.default_rng(63)
    counts = np.array([30000, 1, 50000, 20001], dtype=np.uint32)
    n = int(counts.sum())
    keys = Col(adac, gpu_ctx, rng.integers(0, 5, size=n).astype(np.uint8), counts)
    keep = rng.random(n) < 0.5
    u = (rng.integers(0, 2 ** 40, size=n, dtype=np.uint64) + np.uint64(2 ** 63 - 2 ** 39))
    ucol = Col(adac, gpu_ctx, u, counts)
    q = Quad(gpu_ctx, ucol, ucol, ucol, keys, 4)
    assert any(s >= 2 ** 32 for s in q.expected()[0])
    for k in (None, keep):
        q.check_three_ways(adac, k, "u64 cubed")
    neg = -(rng.integers(0, 2 ** 40, size=n, dtype=np.int64) + np.int64(2 ** 62))
    pos = rng.integers(0, 2 ** 41, size=n, dtype=np.int64) + np.int64(2 ** 62)
    pos[::3] = -pos[::3]
    mix = rng.integers(0, 2 ** 39, size=n, dtype=np.int64) + np.int64(2 ** 62 - 2 ** 38)
    mix[1::2] = -mix[1::2]
    q = Quad(gpu_ctx, Col(adac, gpu_ctx, neg, counts), Col(adac, gpu_ctx, pos, counts), Col(adac, gpu_ctx, mix, counts),
             keys, 4)
    for k in (None, keep):
        q.check_three_ways(adac, k, "int64 x int64 x int64")


# ---------------------------------------------------------------------------------------------------------------------
# 3. both forms at every walk width of a
# ---------------------------------------------------------------------------------------------------------------------
WIDTH_PAIRS = ((1, 32), (32, 1), (13, 7), (7, 13), (32, 32))   # (wb, wc): the lanes-per-round bound takes the wider one


def staged_columns(adac, ctx, rng, counts):
    """{width: a uint32 column packed at exactly that width on `counts`} for every width of WIDTH_PAIRS"""
    return {w: Col(adac, ctx, column_at_width(rng, np.uint32, counts, w, 0 if w == 32 else 1000), counts)
            for w in sorted({w for pair in WIDTH_PAIRS for w in pair})}


@pytest.mark.parametrize("adtype", [np.uint32, np.int32, np.uint64, np.uint16])
def test_both_forms_at_every_walk_width(adac, gpu_ctx, adtype):
    adtype = np.dtype(adtype)
    rng = np.random.default_rng(3410 + adtype.itemsize)
    widths, counts, vals = every_width_column(rng, adtype)
    a = Col(adac, gpu_ctx, vals, counts)
    assert sorted(set(a.widths())) == widths
    n = len(vals)
    keep = rng.random(n) < 0.5
    keep[: n // 2] = clustered(rng, n)[: n // 2]   # the first half in runs of whole words
    bcols = staged_columns(adac, gpu_ctx, rng, counts)
    ccols = staged_columns(adac, gpu_ctx, rng, counts)   # other values at the same widths
    kcols = {wk: Col(adac, gpu_ctx, rng.integers(0, 2 ** wk, size=n).astype(np.uint8), counts) for wk in (1, 3, 5, 8)}
    for wb, wc in WIDTH_PAIRS:
        assert set(bcols[wb].widths()) == {wb} and set(ccols[wc].widths()) == {wc}
        for wk, k in kcols.items():
            assert set(k.widths()) <= {wk, wk + 1}
            q = Quad(gpu_ctx, a, bcols[wb], ccols[wc], k, 7)
            forms = q.forms()   # frames inside [0, 2^32) are the walk's: every segment of the two unsigned narrow types
            if wk <= 5:
                assert (forms["generic"] == 0) if adtype.name in ("uint32", "uint16") else (forms["fast"] == 0), forms
            q.check_three_ways(adac, keep, (wb, wc, wk, "masked"))
            if (wb, wc) in ((7, 13), (32, 32)) and wk in (3, 8):
                q.check_three_ways(adac, None, (wb, wc, wk, "NULL mask"))


@pytest.mark.parametrize("adtype", [np.uint32, np.uint64])
def test_the_walk_at_width_32(adac, gpu_ctx, adtype):
    """`a` spans the whole of [0, 2^32): raw slots of uint32, and uint64 packed at width 32 with frame 0 — both the
    register walk's (four rows per chunk, the keys always out of two dwords)."""
    adtype = np.dtype(adtype)
    rng = np.random.default_rng(33200 + adtype.itemsize)
    counts = np.array([30000, 129, 65534, 7, 4097], dtype=np.uint32)
    n = int(counts.sum())
    a = Col(adac, gpu_ctx, column_at_width(rng, adtype, counts, 32, 0), counts)
    assert set(a.widths()) == {32}
    keep = rng.random(n) < 0.5
    keep[: n // 2] = clustered(rng, n)[: n // 2]
    bcols, ccols = staged_columns(adac, gpu_ctx, rng, counts), staged_columns(adac, gpu_ctx, rng, counts)
    for wb, wc in WIDTH_PAIRS:
        for wk in (1, 3, 5, 8):
            k = Col(adac, gpu_ctx, column_at_width(rng, np.uint8, counts, wk, 0), counts)
            q = Quad(gpu_ctx, a, bcols[wb], ccols[wc], k, 7)
            assert q.forms()["generic"] == 0 and q.forms()["fast"] > 0, (wb, wc, wk, q.forms())
            q.check_three_ways(adac, keep, (wb, wc, wk, "masked"))
            q.check_three_ways(adac, None, (wb, wc, wk, "NULL mask"))


# ---------------------------------------------------------------------------------------------------------------------
# 4. a column whose segments alternate between the two forms; the hand-over word under alternating entry points
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_column_and_alternating_entry_points(adac, gpu_ctx):
    rng = np.random.default_rng(35150)
    vals, keys, counts = mixed_product_column(rng)
    n = len(vals)
    a = Col(adac, gpu_ctx, vals, counts)
    assert a.widths()[:5] == [2, 40, 13, 1, 24]
    b = Col(adac, gpu_ctx, rng.integers(0, 11, size=n).astype(np.uint8), counts)
    c = Col(adac, gpu_ctx, rng.integers(0, 9, size=n).astype(np.int16), counts)
    k = Col(adac, gpu_ctx, keys, counts)
    q = Quad(gpu_ctx, a, b, c, k, 6)
    forms = q.forms()
    assert forms["generic"] > 0 and forms["fast"] > 0, forms
    masks = {"half": rng.random(n) < 0.5, "clustered": clustered(rng, n), "NULL": None}
    for name, keep in masks.items():
        q.check_three_ways(adac, keep, name)
    # the other grouped entry points on the same `a` layout share the partial buffer and the two hand-over slots
    keep = masks["half"]
    d_mask = q.upload_mask(keep)
    exp3 = q.expected(keep)
    exp2 = reference2(vals, b.vals, keys, 6, keep)
    exp_sum = tuple(reference_groups(vals[keep], keys[keep], 6))
    d_s, d_c = gpu_ctx.alloc(7 * 8), gpu_ctx.alloc(7 * 8)

    def poisoned():
        d_s.upload(np.full(7, POISON, dtype=np.uint64))
        d_c.upload(np.full(7, POISON, dtype=np.uint64))

    def group_sum():
        poisoned()
        a.lay.scan_group_sum_valid(a.words, k.lay, k.words, d_mask, 6, d_s, d_c)
        return d_s.download(np.uint64, 7).tolist(), d_c.download(np.uint64, 7).tolist()

    def group_product():
        poisoned()
        a.lay.scan_group_sum_product(a.words, b.lay, b.words, k.lay, k.words, 6, d_s, d_c, d_mask)
        return d_s.download(np.uint64, 7).tolist(), d_c.download(np.uint64, 7).tolist()

    for rw in (1, 0, 1):
        with product3_rw(adac, rw):
            for pattern in ("p3", "3p", "s3s", "33p", "3sp3"):
                for which in pattern:
                    if which == "3":
                        got = q.call(d_mask, rw=rw)
                        assert got[0] == exp3[0] and got[1] == exp3[1], (rw, pattern)
                    elif which == "p":
                        assert group_product() == exp2, (rw, pattern)
                    else:
                        assert group_sum() == exp_sum, (rw, pattern)
    d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 5. every phase of a segment's first bit in its mask word; bits that belong to no row
# ---------------------------------------------------------------------------------------------------------------------
def test_every_mask_phase_and_bits_outside_the_segments(adac, gpu_ctx):
    rng = np.random.default_rng(363)
    vals, keys, counts, voffs, koffs = phase_column(rng)
    assert [int(o) & 63 for o in voffs] == list(range(64))
    boffs = np.cumsum(np.concatenate([[7], counts[:-1] + 3 * np.arange(1, 64)])).astype(np.uint64)
    coffs = np.cumsum(np.concatenate([[21], counts[:-1] + 5 * np.arange(1, 64)])).astype(np.uint64)
    offs = (voffs, boffs, coffs, koffs)
    assert all((x != y).any() for i, x in enumerate(offs) for y in offs[i + 1:])   # four different offset tables
    n = len(vals)
    a = Col(adac, gpu_ctx, vals, counts, voffs)
    b = Col(adac, gpu_ctx, (rng.integers(0, 2 ** 7, size=n) + 3).astype(np.uint16), counts, boffs)
    c = Col(adac, gpu_ctx, (rng.integers(0, 2 ** 5, size=n) - 9).astype(np.int8), counts, coffs)
    k = Col(adac, gpu_ctx, keys, counts, koffs)
    q = Quad(gpu_ctx, a, b, c, k, 7)
    assert q.span % 64 != 0   # the last word has a tail
    for seed in range(2):
        q.check_three_ways(adac, np.random.default_rng(seed).random(n) < 0.5, seed)
    q.check_three_ways(adac, np.ones(n, dtype=bool), "ones")
    # the mask as a 16-byte-aligned slice inside a larger buffer: gaps, tail and sentinel words clear, then all set
    keep = rng.random(n) < 0.5
    exp = q.expected(keep)
    for outside in (False, True):
        words = element_mask(keep, counts, voffs, q.span, outside)
        assert len(words) == (q.span + 63) // 64
        sentinel = np.full(2, 0xFFFFFFFFFFFFFFFF if outside else 0, dtype=np.uint64)
        d_big = gpu_ctx.upload(np.concatenate([sentinel, words, sentinel]))
        for rw in (1, 0):
            with product3_rw(adac, rw):
                got = q.call(d_big.ptr + 16, rw=rw)
                assert got[0] == exp[0] and got[1] == exp[1], (outside, rw)
        d_big.free()


# ---------------------------------------------------------------------------------------------------------------------
# 6. gapped layouts on all four sides; 7. aliasing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adtype,bdtype,cdtype,kdtype,ngroups,vbits,key_top",
                         [(np.int32, np.uint16, np.uint8, np.uint8, 4, 21, 4),
                          (np.uint32, np.uint8, np.uint16, np.uint8, 7, 19, 9),
                          (np.int64, np.int32, np.int8, np.int16, 200, 33, 200)])
def test_gapped_layouts(adac, gpu_ctx, adtype, bdtype, cdtype, kdtype, ngroups, vbits, key_top):
    rng = np.random.default_rng(399)
    counts = np.array([1000, 37, 5000, 2048, 1, 16385], dtype=np.uint32)
    aoffs = np.cumsum(np.concatenate([[3], counts[:-1] + 5]).astype(np.uint64))
    boffs = np.cumsum(np.concatenate([[0], counts[:-1] + 9]).astype(np.uint64))
    coffs = np.cumsum(np.concatenate([[11], counts[:-1] + 70]).astype(np.uint64))
    koffs = np.cumsum(np.concatenate([[1], counts[:-1] + 2]).astype(np.uint64))
    n = int(counts.sum())
    avals, keys = make_case(rng, adtype, kdtype, n, vbits, key_top)
    bvals, _ = make_case(rng, bdtype, kdtype, n, 5, key_top)
    cvals, _ = make_case(rng, cdtype, kdtype, n, 4, key_top)
    q = Quad(gpu_ctx, Col(adac, gpu_ctx, avals, counts, aoffs), Col(adac, gpu_ctx, bvals, counts, boffs),
             Col(adac, gpu_ctx, cvals, counts, coffs), Col(adac, gpu_ctx, keys, counts, koffs), ngroups)
    for name, keep in mask_shapes(rng, counts).items():
        q.check_three_ways(adac, keep, name)
        q.check(keep, (name, "gap bits set"), outside=True)
    q.check_three_ways(adac, None, "NULL")


@pytest.mark.parametrize("adtype,base", [(np.uint32, 70000), (np.int16, -3000), (np.uint64, 2 ** 40)])
def test_aliased_layouts_give_cubes_and_squares_times_c(adac, gpu_ctx, adtype, base):
    rng = np.random.default_rng(32)
    counts = np.array([40000, 129, 65534], dtype=np.uint32)
    n = int(counts.sum())
    vals = (rng.integers(0, 2 ** 11, size=n).astype(np.int64) + base).astype(adtype)
    a = Col(adac, gpu_ctx, vals, counts)
    c = Col(adac, gpu_ctx, rng.integers(-20, 90, size=n).astype(np.int8), counts)
    k = Col(adac, gpu_ctx, rng.integers(0, 6, size=n).astype(np.uint8), counts)
    cubes, squares = Quad(gpu_ctx, a, a, a, k, 6), Quad(gpu_ctx, a, a, c, k, 6)
    assert cubes.expected()[0] == reference(vals, vals, vals, k.vals, 6)[0]
    for keep in (None, rng.random(n) < 0.3):
        cubes.check_three_ways(adac, keep, "a == b == c")
        squares.check_three_ways(adac, keep, "a == b != c")


# ---------------------------------------------------------------------------------------------------------------------
# 8. small grids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [1, 3])
def test_small_grids(adac, gpu_ctx, cus):
    rng = np.random.default_rng(37 + cus)
    widths, counts, vals = every_width_column(rng, np.dtype(np.uint32))
    n = len(vals)
    every = Quad(gpu_ctx, Col(adac, gpu_ctx, vals, counts),
                 Col(adac, gpu_ctx, rng.integers(0, 2 ** 9, size=n).astype(np.uint16), counts),
                 Col(adac, gpu_ctx, rng.integers(0, 2 ** 17, size=n).astype(np.uint32), counts),
                 Col(adac, gpu_ctx, rng.integers(0, 8, size=n).astype(np.uint8), counts), 7)
    mvals, mkeys, mcounts = mixed_product_column(rng)
    mixed = Quad(gpu_ctx, Col(adac, gpu_ctx, mvals, mcounts),
                 Col(adac, gpu_ctx, rng.integers(-5, 6, size=len(mvals)).astype(np.int8), mcounts),
                 Col(adac, gpu_ctx, rng.integers(0, 9, size=len(mvals)).astype(np.uint8), mcounts),
                 Col(adac, gpu_ctx, mkeys, mcounts), 6)
    many = Quad(gpu_ctx, every.a, every.b, every.c,
                Col(adac, gpu_ctx, rng.integers(0, 300, size=n).astype(np.uint16), counts), 256)
    for q in (every, mixed, many):
        keep = rng.random(len(q.a.vals)) < 0.5
        try:
            adac.set_tuning("num_cus", cus)
            q.check_three_ways(adac, keep, cus)
            q.check_three_ways(adac, None, (cus, "NULL"))
        finally:
            adac.set_tuning("num_cus", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 9. Q1 end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_q1_sum_charge(adac, gpu_ctx):
    """WHERE l_shipdate <= cutoff; SUM(l_extendedprice * (1 - l_discount) * (1 + l_tax)) GROUP BY the flag code, in
    integer decimals: 10000 SUM(p) + 100 SUM(p t) - 100 SUM(p d) - SUM(p d t) == numpy's SUM(p (100 - d)(100 + t))."""
    rng = np.random.default_rng(31998)
    n = 200_000
    counts = np.array([65534] * (n // 65534) + [n % 65534], dtype=np.uint32)
    code = rng.choice(6, size=n, p=[.25, .25, .01, .24, .24, .01]).astype(np.uint8)
    price = rng.integers(90_000, 10_500_000, size=n).astype(np.int32)
    qty = rng.integers(1, 51, size=n).astype(np.int32)
    disc = rng.integers(0, 11, size=n).astype(np.int32)
    tax = rng.integers(0, 9, size=n).astype(np.int32)
    date = rng.integers(8036, 10562, size=n).astype(np.int32)
    cutoff = 10471
    col = lambda v: Col(adac, gpu_ctx, v, counts)
    d, qc, p, dc, tc, k = col(date), col(qty), col(price), col(disc), col(tax), col(code)
    d_bm = gpu_ctx.alloc((n + 63) // 64 * 8)
    d_sel = gpu_ctx.alloc(len(counts) * 8)
    int_min = int(np.array([np.iinfo(np.int32).min]).view(np.uint32)[0])
    d.lay.scan_select_between(d.words, int_min, cutoff, d_bm, d_sel)
    m = date <= cutoff
    assert int(d_sel.download(np.uint64, len(counts)).sum()) == int(m.sum()) and 0.8 * n < m.sum() < n
    bins = [m & (code == g) for g in range(6)]
    d_s, d_c = gpu_ctx.alloc(7 * 8), gpu_ctx.alloc(7 * 8)

    def group_sum(v):
        v.lay.scan_group_sum_valid(v.words, k.lay, k.words, d_bm, 6, d_s, d_c)
        return d_s.download(np.uint64, 7).tolist(), d_c.download(np.uint64, 7).tolist()

    def group_product(x, y):
        x.lay.scan_group_sum_product(x.words, y.lay, y.words, k.lay, k.words, 6, d_s, None, d_bm)
        return d_s.download(np.uint64, 7).tolist()

    (sum_q, cnt_q), (sum_p, cnt_p), (sum_d, cnt_d) = group_sum(qc), group_sum(p), group_sum(dc)
    sum_pd, sum_pt = group_product(p, dc), group_product(p, tc)
    rows = [int(b.sum()) for b in bins] + [0]
    assert cnt_q == cnt_p == cnt_d == rows
    assert sum_q[:6] == [int(qty[b].sum(dtype=np.int64)) for b in bins]
    assert sum_d[:6] == [int(disc[b].sum(dtype=np.int64)) for b in bins]
    p64, d64, t64 = price.astype(np.int64), disc.astype(np.int64), tax.astype(np.int64)
    assert [100 * sum_p[g] - sum_pd[g] for g in range(6)] == [int((p64[b] * (100 - d64[b])).sum()) for b in bins]
    q = Quad(gpu_ctx, p, dc, tc, k, 6)
    forms = q.forms()
    assert forms["fast"] > 0 and forms["generic"] == 0, forms   # Q1's columns are the register walk's
    exp = [int((p64[b] * (100 - d64[b]) * (100 + t64[b])).sum()) for b in bins]
    for rw in (1, 0):
        with product3_rw(adac, rw):
            sum_pdt, cnt = q.call(d_bm, rw=rw)
            charge = [10000 * sum_p[g] + 100 * sum_pt[g] - 100 * sum_pd[g] - sum_pdt[g] for g in range(6)]
            assert charge == exp, rw
            assert cnt == cnt_p == rows, rw   # the masked grouped SUM's counts
            assert sum_pdt[6] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals; 11. layouts without rows
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(adac, gpu_ctx):
    counts = np.array([10, 20], dtype=np.uint32)
    a = adac.Layout(gpu_ctx, np.uint32, counts)
    b = adac.Layout(gpu_ctx, np.int16, counts)
    c = adac.Layout(gpu_ctx, np.int32, counts)
    k = adac.Layout(gpu_ctx, np.uint8, counts)
    other = adac.Layout(gpu_ctx, np.uint8, np.array([10, 21], dtype=np.uint32))
    d = gpu_ctx.alloc(4096).zero()
    ctx2 = adac.Context(0)
    try:
        far = adac.Layout(ctx2, np.uint8, counts)
        far_b, far_c, far_k = (adac.Layout(ctx2, t, counts) for t in (np.int16, np.int32, np.uint8))
        p3 = lambda *args: (lambda: args[0].scan_group_sum_product3(*args[1:]))
        unbound = adac.Layout.scan_group_sum_product3
        refused = {
            "NULL a": lambda: unbound(NullLayout, d, b, d, c, d, k, d, 4, d, d),
            "NULL b": p3(a, d, NullLayout, d, c, d, k, d, 4, d, d),
            "NULL c": p3(a, d, b, d, NullLayout, d, k, d, 4, d, d),
            "NULL keys": p3(a, d, b, d, c, d, NullLayout, d, 4, d, d),
            "a on another context": p3(far, d, b, d, c, d, k, d, 4, d, d),
            "b on another context": p3(a, d, far, d, c, d, k, d, 4, d, d),
            "c on another context": p3(a, d, b, d, far, d, k, d, 4, d, d),
            "keys on another context": p3(a, d, b, d, c, d, far, d, 4, d, d),
            "only a on this context": p3(a, d, far_b, d, far_c, d, far_k, d, 4, d, d),
            "counts of a": p3(other, d, b, d, c, d, k, d, 4, d, d),
            "counts of b": p3(a, d, other, d, c, d, k, d, 4, d, d),
            "counts of c": p3(a, d, b, d, other, d, k, d, 4, d, d),
            "counts of keys": p3(a, d, b, d, c, d, other, d, 4, d, d),
            "ngroups 0": p3(a, d, b, d, c, d, k, d, 0, d, d),
            "ngroups 257": p3(a, d, b, d, c, d, k, d, 257, d, d),
            "NULL d_sums": p3(a, d, b, d, c, d, k, d, 4, None, d),
            "NULL a words": p3(a, None, b, d, c, d, k, d, 4, d, d),
            "NULL b words": p3(a, d, b, None, c, d, k, d, 4, d, d),
            "NULL c words": p3(a, d, b, d, c, None, k, d, 4, d, d),
            "NULL key words": p3(a, d, b, d, c, d, k, None, 4, d, d),
            "a words off by 8": p3(a, d.ptr + 8, b, d, c, d, k, d, 4, d, d),
            "b words off by 8": p3(a, d, b, d.ptr + 8, c, d, k, d, 4, d, d),
            "c words off by 8": p3(a, d, b, d, c, d.ptr + 8, k, d, 4, d, d),
            "key words off by 8": p3(a, d, b, d, c, d, k, d.ptr + 8, 4, d, d),
        }
        for what, call in refused.items():
            with pytest.raises(adac.AdacError) as e:
                call()
            assert e.value.status == INVALID_ARGUMENT, what
        for lay in (far, far_b, far_c, far_k):
            lay.close()
    finally:
        ctx2.close()


def test_layouts_without_rows_write_zeros(adac, gpu_ctx):
    for counts in (np.array([0, 0, 0], dtype=np.uint32), np.array([0], dtype=np.uint32)):
        a = adac.Layout(gpu_ctx, np.int32, counts)
        b = adac.Layout(gpu_ctx, np.uint8, counts)
        c = adac.Layout(gpu_ctx, np.int64, counts)
        k = adac.Layout(gpu_ctx, np.uint8, counts)
        for ngroups in (1, 6, 256):
            d_s, d_c = gpu_ctx.alloc((ngroups + 2) * 8), gpu_ctx.alloc((ngroups + 2) * 8)
            for words in (None, gpu_ctx.alloc(64).zero()):
                for d_counts in (d_c, None):
                    d_s.upload(np.full(ngroups + 2, POISON, dtype=np.uint64))
                    d_c.upload(np.full(ngroups + 2, POISON, dtype=np.uint64))
                    a.scan_group_sum_product3(words, b, words, c, words, k, words, ngroups, d_s, d_counts)
                    assert d_s.download(np.uint64, ngroups + 2).tolist() == [0] * (ngroups + 1) + [POISON]
                    exp_c = [0] * (ngroups + 1) + [POISON] if d_counts is not None else [POISON] * (ngroups + 2)
                    assert d_c.download(np.uint64, ngroups + 2).tolist() == exp_c
                    assert a.debug_group_handover() == 0
