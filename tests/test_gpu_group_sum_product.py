"""adac_scan_group_sum_product: SUM(a * b) GROUP BY key over three packed columns of one table under a selection bitmap
indexed in a's element space (Q1's sum_disc_price = 100 SUM(price) - SUM(price * disc) per group).

The expected value is numpy over the ORIGINAL columns: each of a and b widened to 64 bits by its own signedness and
viewed as uint64, multiplied (uint64 wraps mod 2^64, as the ABI says), grouped by the key as an unsigned number of its own
width (keys >= ngroups in bin `ngroups`), summed with dtype=uint64.  Compared exactly.  Both kernel forms are held to it:
the register walk (k_group_product_rw) with the staged kernel (k_group_product) for what it leaves, and the staged kernel
alone under group_product_rw = 0.  Results are poisoned before every call.  Which kernel took what is read back after
the calls (adac_debug_group_handover: the scan groups the register walk left) and held against the host mirror of the
eligibility rule, so the walk cannot quietly hand its work to the staged kernel."""
import importlib

import numpy as np
import pytest

from test_gpu_group_sum import encode_column, reference_groups
from test_gpu_group_sum_rw import every_width_column, mixed_walk_column
from test_gpu_group_sum_valid import clustered, dense_offsets, element_mask, make_case, mask_shapes, phase_column

group_product_form_groups = importlib.import_module("duckdb-adaptive-compression_amd.forms").group_product_form_groups
pytestmark = pytest.mark.gpu

ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
POISON = 0xDEADBEEFDEADBEEF
INVALID_ARGUMENT = 1


class product_rw:
    """with product_rw(adac, 0): the staged kernel alone; the default (1) restored on exit."""

    def __init__(self, adac, value):
        self.adac, self.value = adac, value

    def __enter__(self):
        self.adac.set_tuning("group_product_rw", self.value)

    def __exit__(self, *exc):
        self.adac.set_tuning("group_product_rw", 1)


def widen(v):
    return v.astype(np.int64 if v.dtype.kind == "i" else np.uint64).view(np.uint64)


def reference(a, b, keys, ngroups, keep=None):
    """(sums, counts), ngroups + 1 entries each"""
    p = widen(a) * widen(b)
    ukeys = keys.view(np.dtype("u%d" % keys.dtype.itemsize)).astype(np.uint64)
    bins = np.minimum(ukeys, np.uint64(ngroups)).astype(np.int64)
    if keep is not None:
        p, bins = p[keep], bins[keep]
    sums = [int(p[bins == g].sum(dtype=np.uint64)) for g in range(ngroups + 1)]
    cnts = np.bincount(bins, minlength=ngroups + 1).tolist()
    return sums, cnts


class Col:
    """A column encoded on `counts` rows per segment (at element offsets `offs`, default back to back)."""

    def __init__(self, adac, ctx, vals, counts, offs=None):
        self.vals, self.counts = vals, counts
        self.offs = dense_offsets(counts) if offs is None else offs
        self.lay, self.words = encode_column(adac, ctx, vals, counts, offs)

    def widths(self):
        return self.lay.get_descs()["width"].tolist()


class Triple:
    def __init__(self, ctx, a, b, k, ngroups):
        self.ctx, self.a, self.b, self.k, self.ngroups = ctx, a, b, k, ngroups
        self.span = int(a.lay.value_span)
        self.d_sums, self.d_cnts = ctx.alloc((ngroups + 2) * 8), ctx.alloc((ngroups + 2) * 8)
        self._forms = None

    def left_to_the_staged_kernel(self, rw=1):
        """what the register walk of a call hands over, by the host mirror: the scan groups it cannot take; nothing when
        it is not launched (knob at 0, more than 8 bins: the staged kernel then takes everything)"""
        if self._forms is None:
            self._forms = self.forms()
        return self._forms["generic"] if rw and self.ngroups + 1 <= 8 else 0

    def call(self, d_mask=None, counts=True):
        """-> (sums, counts or None); nothing is written past ngroups + 1 entries"""
        n = self.ngroups + 1
        self.d_sums.upload(np.full(n + 1, POISON, dtype=np.uint64))
        self.d_cnts.upload(np.full(n + 1, POISON, dtype=np.uint64))
        self.a.lay.scan_group_sum_product(self.a.words, self.b.lay, self.b.words, self.k.lay, self.k.words, self.ngroups,
                                          self.d_sums, self.d_cnts if counts else None, d_mask)
        s, c = self.d_sums.download(np.uint64, n + 1).tolist(), self.d_cnts.download(np.uint64, n + 1).tolist()
        assert s[n] == POISON and c[n] == POISON
        if not counts:
            assert c == [POISON] * (n + 1)
        return s[:n], (c[:n] if counts else None)

    def forms(self):
        """{"fast": scan groups of a the register walk takes, "generic": the rest} by the host mirror of the rule"""
        kind = lambda c: (c.vals.dtype.itemsize, c.vals.dtype.kind == "i")
        return group_product_form_groups(self.a.lay.get_descs(), self.b.lay.get_descs(), self.k.lay.get_descs(),
                                         self.ngroups, kind(self.a), kind(self.b), self.k.vals.dtype.itemsize)

    def upload_mask(self, keep, outside=False):
        return self.ctx.upload(element_mask(keep, self.a.counts, self.a.offs, self.span, outside))

    def expected(self, keep=None):
        return reference(self.a.vals, self.b.vals, self.k.vals, self.ngroups, keep)

    def check(self, keep, what, outside=False):
        """One masked call against numpy (keep None: the NULL mask); the counts add up to the kept rows; without
        d_counts the same sums."""
        d_mask = None if keep is None else self.upload_mask(keep, outside)
        exp = self.expected(keep)
        got = self.call(d_mask)
        assert got[0] == exp[0] and got[1] == exp[1], what
        assert sum(got[1]) == (len(self.a.vals) if keep is None else int(keep.sum())), what
        assert self.a.lay.debug_group_handover() == self.left_to_the_staged_kernel(), what
        assert self.call(d_mask, counts=False) == (exp[0], None), (what, "no counts")
        assert self.a.lay.debug_group_handover() == self.left_to_the_staged_kernel(), (what, "no counts")
        if d_mask is not None:
            d_mask.free()
        return got

    def check_three_ways(self, adac, keep, what):
        """The register walk, the staged kernel alone, the register walk again (the hand-over word was left at zero)."""
        d_mask = None if keep is None else self.upload_mask(keep)
        exp = self.expected(keep)
        for rw in (1, 0, 1):
            with product_rw(adac, rw):
                got = self.call(d_mask)
                assert got[0] == exp[0] and got[1] == exp[1], (what, rw)
                assert self.a.lay.debug_group_handover() == self.left_to_the_staged_kernel(rw), (what, rw)
                assert self.call(d_mask, counts=False)[0] == exp[0], (what, rw, "no counts")
                assert self.a.lay.debug_group_handover() == self.left_to_the_staged_kernel(rw), (what, rw, "no counts")
        if d_mask is not None:
            d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 1. types and masks
# ---------------------------------------------------------------------------------------------------------------------
COUNTS1 = np.array([2048, 32767, 1, 0, 5000, 70001, 63, 4096], dtype=np.uint32)
KEY_CASES = ((np.uint8, 6, 6), (np.uint16, 40, 50), (np.int32, 256, 300))
B_TYPES = (np.uint8, np.int16, np.int32, np.uint64)
_shared = {}


def shared_columns(adac, ctx):
    """b and key columns on COUNTS1, encoded once for all the types of a"""
    if not _shared:
        rng = np.random.default_rng(4242)
        n = int(COUNTS1.sum())
        for bt in B_TYPES:
            tb = 8 * np.dtype(bt).itemsize
            vals, _ = make_case(rng, bt, np.uint8, n, tb // 2 + 1, 2)
            _shared["b", np.dtype(bt).name] = Col(adac, ctx, vals, COUNTS1)
        for kt, ngroups, key_top in KEY_CASES:
            _, keys = make_case(rng, np.uint8, kt, n, 4, key_top)
            _shared["k", np.dtype(kt).name] = Col(adac, ctx, keys, COUNTS1)
    return _shared


@pytest.mark.parametrize("adtype", ALL)
def test_every_type_of_a_under_every_mask_shape(adac, gpu_ctx, adtype):
    adtype = np.dtype(adtype)
    cols = shared_columns(adac, gpu_ctx)
    rng = np.random.default_rng(880 + adtype.itemsize + (adtype.kind == "i"))
    shapes = mask_shapes(np.random.default_rng(11), COUNTS1)
    shapes["NULL"] = None
    tb = 8 * adtype.itemsize
    for vbits in (6, tb // 2 + 1):
        vals, _ = make_case(rng, adtype, np.uint8, int(COUNTS1.sum()), vbits, 2)
        a = Col(adac, gpu_ctx, vals, COUNTS1)
        for bt in B_TYPES:
            for kt, ngroups, _ in KEY_CASES:
                t = Triple(gpu_ctx, a, cols["b", np.dtype(bt).name], cols["k", np.dtype(kt).name], ngroups)
                for name, keep in shapes.items():
                    got = t.check(keep, (vbits, np.dtype(bt).name, np.dtype(kt).name, name))
                    if name == "zeros":
                        assert not any(got[0]) and not any(got[1])
                    if name == "ones":
                        assert got[0] == t.expected()[0]


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
    t = Triple(gpu_ctx, ucol, ucol, keys, 4)
    assert any(s >= 2 ** 32 for s in t.expected()[0])
    for k in (None, keep):
        t.check_three_ways(adac, k, "u64 squared")
    neg = -(rng.integers(0, 2 ** 40, size=n, dtype=np.int64) + np.int64(2 ** 62))
    pos = rng.integers(0, 2 ** 41, size=n, dtype=np.int64) + np.int64(2 ** 62)
    pos[::3] = -pos[::3]
    t = Triple(gpu_ctx, Col(adac, gpu_ctx, neg, counts), Col(adac, gpu_ctx, pos, counts), keys, 4)
    for k in (None, keep):
        t.check_three_ways(adac, k, "int64 x int64")


# ---------------------------------------------------------------------------------------------------------------------
# 3. both forms at every walk width of a
# ---------------------------------------------------------------------------------------------------------------------
def column_at_width(rng, dtype, counts, w, base):
    """every segment packed at exactly w bits: its first two rows are the ends of [base, base + 2^w)"""
    n = int(counts.sum())
    f = rng.integers(0, 2 ** w, size=n, dtype=np.uint64)
    for s, c in zip(dense_offsets(counts).astype(np.int64), counts):
        if c >= 2:
            f[s], f[s + 1] = 0, 2 ** w - 1
    return (f + np.uint64(base)).astype(dtype)


@pytest.mark.parametrize("adtype", [np.uint32, np.int32, np.uint64, np.uint16])
def test_both_forms_at_every_walk_width(adac, gpu_ctx, adtype):
    adtype = np.dtype(adtype)
    rng = np.random.default_rng(410 + adtype.itemsize)
    widths, counts, vals = every_width_column(rng, adtype)
    a = Col(adac, gpu_ctx, vals, counts)
    assert sorted(set(a.widths())) == widths
    n = len(vals)
    keep = rng.random(n) < 0.5
    keep[: n // 2] = clustered(rng, n)[: n // 2]   # the first half in runs of whole words
    bcols = {wb: Col(adac, gpu_ctx, column_at_width(rng, np.uint32, counts, wb, 0 if wb == 32 else 1000), counts)
             for wb in (1, 7, 13, 32)}
    kcols = {wk: Col(adac, gpu_ctx, rng.integers(0, 2 ** wk, size=n).astype(np.uint8), counts) for wk in (1, 3, 5, 8)}
    for wb, b in bcols.items():
        assert set(b.widths()) == {wb}
        for wk, k in kcols.items():
            assert set(k.widths()) <= {wk, wk + 1}
            t = Triple(gpu_ctx, a, b, k, 7)
            forms = t.forms()   # frames inside [0, 2^32) are the walk's: every segment of the two unsigned narrow types
            if wk <= 5:
                assert (forms["generic"] == 0) if adtype.name in ("uint32", "uint16") else (forms["fast"] == 0), forms
            t.check_three_ways(adac, keep, (wb, wk, "masked"))
            if wb in (7, 32) and wk in (3, 8):
                t.check_three_ways(adac, None, (wb, wk, "NULL mask"))


@pytest.mark.parametrize("adtype", [np.uint32, np.uint64])
def test_the_walk_at_width_32(adac, gpu_ctx, adtype):
    """every_width_column stops below the type's width and gives a 64-bit type frames far above 2^32, so its width-32
    segments are the staged kernel's.  Here `a` spans the whole of [0, 2^32): raw slots of uint32, and uint64 packed at
    width 32 with frame 0 — both the register walk's (four rows per chunk, the keys always out of two dwords)."""
    adtype = np.dtype(adtype)
    rng = np.random.default_rng(3200 + adtype.itemsize)
    counts = np.array([30000, 129, 65534, 7, 4097], dtype=np.uint32)
    n = int(counts.sum())
    a = Col(adac, gpu_ctx, column_at_width(rng, adtype, counts, 32, 0), counts)
    assert set(a.widths()) == {32}
    keep = rng.random(n) < 0.5
    keep[: n // 2] = clustered(rng, n)[: n // 2]
    for wb in (1, 7, 13, 32):
        b = Col(adac, gpu_ctx, column_at_width(rng, np.uint32, counts, wb, 0 if wb == 32 else 1000), counts)
        assert set(b.widths()) == {wb}
        for wk in (1, 3, 5, 8):
            k = Col(adac, gpu_ctx, column_at_width(rng, np.uint8, counts, wk, 0), counts)
            t = Triple(gpu_ctx, a, b, k, 7)
            assert t.forms()["generic"] == 0 and t.forms()["fast"] > 0, (wb, wk, t.forms())
            t.check_three_ways(adac, keep, (wb, wk, "masked"))
            t.check_three_ways(adac, None, (wb, wk, "NULL mask"))


# ---------------------------------------------------------------------------------------------------------------------
# 4. a column whose segments alternate between the two forms; the hand-over word under alternating entry points
# ---------------------------------------------------------------------------------------------------------------------
def mixed_product_column(rng):
    """mixed_walk_column's shape (int64: widths 2, 40, 13, 1, 24, raw 64, a segment that wraps, 6) with frames of
    reference inside [0, 2^32) on the segments at widths 13, 24 and 6: the latter two are the register walk's, the rest —
    widths outside 4..32, a frame at 2^50, keys at width 10, raw signed slots, the wrapping segment — the staged kernel's."""
    vals, keys, counts = mixed_walk_column(rng)
    starts = dense_offsets(counts).astype(np.int64)
    for seg, old, new in ((2, -50000, 50000), (4, 1 << 33, 1 << 20), (7, -300, 300)):
        s, c = int(starts[seg]), int(counts[seg])
        vals[s:s + c] += new - old
    return vals, keys, counts


@pytest.mark.parametrize("column", [mixed_walk_column, mixed_product_column])
def test_mixed_column_and_alternating_entry_points(adac, gpu_ctx, column):
    rng = np.random.default_rng(5150)
    vals, keys, counts = column(rng)
    n = len(vals)
    a = Col(adac, gpu_ctx, vals, counts)
    assert a.widths()[:5] == [2, 40, 13, 1, 24]
    b = Col(adac, gpu_ctx, rng.integers(0, 11, size=n).astype(np.uint8), counts)
    k = Col(adac, gpu_ctx, keys, counts)
    t = Triple(gpu_ctx, a, b, k, 6)
    forms = t.forms()
    assert forms["generic"] > 0 and (forms["fast"] > 0) == (column is mixed_product_column), forms
    masks = {"half": rng.random(n) < 0.5, "clustered": clustered(rng, n), "NULL": None}
    for name, keep in masks.items():
        t.check_three_ways(adac, keep, name)
    # adac_scan_group_sum_valid on the same `a` layout shares the partial buffer and the two hand-over slots
    keep = masks["half"]
    d_mask = t.upload_mask(keep)
    exp = t.expected(keep)
    exp_sum = tuple(reference_groups(vals[keep], keys[keep], 6))
    d_s, d_c = gpu_ctx.alloc(7 * 8), gpu_ctx.alloc(7 * 8)

    def group_sum():
        d_s.upload(np.full(7, POISON, dtype=np.uint64))
        d_c.upload(np.full(7, POISON, dtype=np.uint64))
        a.lay.scan_group_sum_valid(a.words, k.lay, k.words, d_mask, 6, d_s, d_c)
        return d_s.download(np.uint64, 7).tolist(), d_c.download(np.uint64, 7).tolist()

    for rw in (1, 0, 1):
        with product_rw(adac, rw):
            for pattern in ("ps", "pps", "pss", "spsp"):
                for which in pattern:
                    if which == "p":
                        got = t.call(d_mask)
                        assert got[0] == exp[0] and got[1] == exp[1], (rw, pattern)
                    else:
                        assert group_sum() == exp_sum, (rw, pattern)
    d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 5. every phase of a segment's first bit in its mask word; bits that belong to no row
# ---------------------------------------------------------------------------------------------------------------------
def test_every_mask_phase_and_bits_outside_the_segments(adac, gpu_ctx):
    rng = np.random.default_rng(63)
    vals, keys, counts, voffs, koffs = phase_column(rng)
    assert [int(o) & 63 for o in voffs] == list(range(64))
    boffs = np.cumsum(np.concatenate([[7], counts[:-1] + 3 * np.arange(1, 64)])).astype(np.uint64)
    assert (voffs != koffs).any() and (voffs != boffs).any() and (koffs != boffs).any()
    n = len(vals)
    a = Col(adac, gpu_ctx, vals, counts, voffs)
    b = Col(adac, gpu_ctx, (rng.integers(0, 2 ** 7, size=n) + 3).astype(np.uint16), counts, boffs)
    k = Col(adac, gpu_ctx, keys, counts, koffs)
    t = Triple(gpu_ctx, a, b, k, 7)
    assert t.span % 64 != 0   # the last word has a tail
    for seed in range(2):
        t.check_three_ways(adac, np.random.default_rng(seed).random(n) < 0.5, seed)
    t.check_three_ways(adac, np.ones(n, dtype=bool), "ones")
    # the mask as a 16-byte-aligned slice inside a larger buffer: gaps, tail and sentinel words clear, then all set
    keep = rng.random(n) < 0.5
    exp = t.expected(keep)
    for outside in (False, True):
        words = element_mask(keep, counts, voffs, t.span, outside)
        assert len(words) == (t.span + 63) // 64
        sentinel = np.full(2, 0xFFFFFFFFFFFFFFFF if outside else 0, dtype=np.uint64)
        d_big = gpu_ctx.upload(np.concatenate([sentinel, words, sentinel]))
        for rw in (1, 0):
            with product_rw(adac, rw):
                got = t.call(d_big.ptr + 16)
                assert got[0] == exp[0] and got[1] == exp[1], (outside, rw)
        d_big.free()


# ---------------------------------------------------------------------------------------------------------------------
# 6. gapped layouts on all three sides; 7. squares
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adtype,bdtype,kdtype,ngroups,vbits,key_top", [(np.int32, np.uint16, np.uint8, 4, 21, 4),
                                                                        (np.uint32, np.uint8, np.uint8, 7, 19, 9),
                                                                        (np.int64, np.int32, np.int16, 200, 33, 200)])
def test_gapped_layouts(adac, gpu_ctx, adtype, bdtype, kdtype, ngroups, vbits, key_top):
    rng = np.random.default_rng(99)
    counts = np.array([1000, 37, 5000, 2048, 1, 16385], dtype=np.uint32)
    aoffs = np.cumsum(np.concatenate([[3], counts[:-1] + 5]).astype(np.uint64))
    boffs = np.cumsum(np.concatenate([[0], counts[:-1] + 9]).astype(np.uint64))
    koffs = np.cumsum(np.concatenate([[1], counts[:-1] + 2]).astype(np.uint64))
    n = int(counts.sum())
    avals, keys = make_case(rng, adtype, kdtype, n, vbits, key_top)
    bvals, _ = make_case(rng, bdtype, kdtype, n, 5, key_top)
    t = Triple(gpu_ctx, Col(adac, gpu_ctx, avals, counts, aoffs), Col(adac, gpu_ctx, bvals, counts, boffs),
               Col(adac, gpu_ctx, keys, counts, koffs), ngroups)
    for name, keep in mask_shapes(rng, counts).items():
        t.check_three_ways(adac, keep, name)
        t.check(keep, (name, "gap bits set"), outside=True)
    t.check_three_ways(adac, None, "NULL")


@pytest.mark.parametrize("adtype,base", [(np.uint32, 70000), (np.int16, -3000), (np.uint64, 2 ** 40)])
def test_a_is_b_gives_the_sum_of_squares(adac, gpu_ctx, adtype, base):
    rng = np.random.default_rng(2)
    counts = np.array([40000, 129, 65534], dtype=np.uint32)
    n = int(counts.sum())
    vals = (rng.integers(0, 2 ** 11, size=n).astype(np.int64) + base).astype(adtype)
    a = Col(adac, gpu_ctx, vals, counts)
    k = Col(adac, gpu_ctx, rng.integers(0, 6, size=n).astype(np.uint8), counts)
    t = Triple(gpu_ctx, a, a, k, 6)
    assert t.expected()[0] == reference(vals, vals, k.vals, 6)[0]
    for keep in (None, rng.random(n) < 0.3):
        t.check_three_ways(adac, keep, "squares")


# ---------------------------------------------------------------------------------------------------------------------
# 8. small grids
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [1, 3])
def test_small_grids(adac, gpu_ctx, cus):
    rng = np.random.default_rng(7 + cus)
    widths, counts, vals = every_width_column(rng, np.dtype(np.uint32))
    n = len(vals)
    every = Triple(gpu_ctx, Col(adac, gpu_ctx, vals, counts),
                   Col(adac, gpu_ctx, rng.integers(0, 2 ** 9, size=n).astype(np.uint16), counts),
                   Col(adac, gpu_ctx, rng.integers(0, 8, size=n).astype(np.uint8), counts), 7)
    mvals, mkeys, mcounts = mixed_product_column(rng)
    mixed = Triple(gpu_ctx, Col(adac, gpu_ctx, mvals, mcounts),
                   Col(adac, gpu_ctx, rng.integers(-5, 6, size=len(mvals)).astype(np.int8), mcounts),
                   Col(adac, gpu_ctx, mkeys, mcounts), 6)
    many = Triple(gpu_ctx, every.a, every.b, Col(adac, gpu_ctx, rng.integers(0, 300, size=n).astype(np.uint16), counts), 256)
    for t in (every, mixed, many):
        keep = rng.random(len(t.a.vals)) < 0.5
        try:
            adac.set_tuning("num_cus", cus)
            t.check_three_ways(adac, keep, cus)
            t.check_three_ways(adac, None, (cus, "NULL"))
        finally:
            adac.set_tuning("num_cus", 0)


# ---------------------------------------------------------------------------------------------------------------------
# 9. Q1 end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_q1_sum_disc_price(adac, gpu_ctx):
    """WHERE l_shipdate <= cutoff; SUM(l_extendedprice * (1 - l_discount)) GROUP BY the flag code, in integer decimals:
    100 * SUM(price) - SUM(price * disc) == numpy's SUM(price * (100 - disc)) per group."""
    rng = np.random.default_rng(1998)
    n = 200_000
    counts = np.array([65534] * (n // 65534) + [n % 65534], dtype=np.uint32)
    code = rng.choice(6, size=n, p=[.25, .25, .01, .24, .24, .01]).astype(np.uint8)
    price = rng.integers(90_000, 10_500_000, size=n, dtype=np.int64)
    disc = rng.integers(0, 11, size=n).astype(np.int8)
    date = rng.integers(8036, 10562, size=n).astype(np.int32)
    cutoff = 10471
    d = Col(adac, gpu_ctx, date, counts)
    p, dc, k = Col(adac, gpu_ctx, price, counts), Col(adac, gpu_ctx, disc, counts), Col(adac, gpu_ctx, code, counts)
    d_bm = gpu_ctx.alloc((n + 63) // 64 * 8)
    d_sel = gpu_ctx.alloc(len(counts) * 8)
    int_min = int(np.array([np.iinfo(np.int32).min]).view(np.uint32)[0])
    d.lay.scan_select_between(d.words, int_min, cutoff, d_bm, d_sel)
    m = date <= cutoff
    assert int(d_sel.download(np.uint64, len(counts)).sum()) == int(m.sum()) and 0.8 * n < m.sum() < n
    d_s, d_c = gpu_ctx.alloc(7 * 8), gpu_ctx.alloc(7 * 8)
    p.lay.scan_group_sum_valid(p.words, k.lay, k.words, d_bm, 6, d_s, d_c)
    sum_price, cnt_price = d_s.download(np.uint64, 7).tolist(), d_c.download(np.uint64, 7).tolist()
    t = Triple(gpu_ctx, p, dc, k, 6)
    forms = t.forms()
    assert forms["fast"] > 0 and forms["generic"] == 0, forms   # Q1's columns are the register walk's
    for rw in (1, 0):
        with product_rw(adac, rw):
            sum_pd, cnt = t.call(d_bm)
            exp = [int((price[m & (code == g)] * (100 - disc[m & (code == g)].astype(np.int64))).sum()) for g in range(6)]
            assert [100 * sum_price[g] - sum_pd[g] for g in range(6)] == exp, rw
            assert cnt == cnt_price == [int((m & (code == g)).sum()) for g in range(6)] + [0], rw
            assert sum_pd[6] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals; a layout without rows
# ---------------------------------------------------------------------------------------------------------------------
class NullLayout:
    _h = None


def test_argument_errors(adac, gpu_ctx):
    counts = np.array([10, 20], dtype=np.uint32)
    a = adac.Layout(gpu_ctx, np.uint32, counts)
    b = adac.Layout(gpu_ctx, np.int16, counts)
    k = adac.Layout(gpu_ctx, np.uint8, counts)
    other = adac.Layout(gpu_ctx, np.uint8, np.array([10, 21], dtype=np.uint32))
    d = gpu_ctx.alloc(4096).zero()
    ctx2 = adac.Context(0)
    try:
        far = adac.Layout(ctx2, np.uint8, counts)
        refused = {
            "NULL a": lambda: adac.Layout.scan_group_sum_product(NullLayout, d, b, d, k, d, 4, d, d),
            "NULL b": lambda: a.scan_group_sum_product(d, NullLayout, d, k, d, 4, d, d),
            "NULL keys": lambda: a.scan_group_sum_product(d, b, d, NullLayout, d, 4, d, d),
            "b on another context": lambda: a.scan_group_sum_product(d, far, d, k, d, 4, d, d),
            "keys on another context": lambda: a.scan_group_sum_product(d, b, d, far, d, 4, d, d),
            "counts of b": lambda: a.scan_group_sum_product(d, other, d, k, d, 4, d, d),
            "counts of keys": lambda: a.scan_group_sum_product(d, b, d, other, d, 4, d, d),
            "counts of b and keys alike, not a's": lambda: other.scan_group_sum_product(d, b, d, k, d, 4, d, d),
            "ngroups 0": lambda: a.scan_group_sum_product(d, b, d, k, d, 0, d, d),
            "ngroups 257": lambda: a.scan_group_sum_product(d, b, d, k, d, 257, d, d),
            "NULL d_sums": lambda: a.scan_group_sum_product(d, b, d, k, d, 4, None, d),
            "NULL a words": lambda: a.scan_group_sum_product(None, b, d, k, d, 4, d, d),
            "NULL b words": lambda: a.scan_group_sum_product(d, b, None, k, d, 4, d, d),
            "NULL key words": lambda: a.scan_group_sum_product(d, b, d, k, None, 4, d, d),
            "a words off by 8": lambda: a.scan_group_sum_product(d.ptr + 8, b, d, k, d, 4, d, d),
            "b words off by 8": lambda: a.scan_group_sum_product(d, b, d.ptr + 8, k, d, 4, d, d),
            "key words off by 8": lambda: a.scan_group_sum_product(d, b, d, k, d.ptr + 8, 4, d, d),
        }
        for what, call in refused.items():
            with pytest.raises(adac.AdacError) as e:
                call()
            assert e.value.status == INVALID_ARGUMENT, what
        far.close()
    finally:
        ctx2.close()


def test_a_layout_without_rows_writes_zeros(adac, gpu_ctx):
    for counts in (np.array([0, 0, 0], dtype=np.uint32), np.array([0], dtype=np.uint32)):
        a = adac.Layout(gpu_ctx, np.int32, counts)
        b = adac.Layout(gpu_ctx, np.uint8, counts)
        k = adac.Layout(gpu_ctx, np.uint8, counts)
        for ngroups in (1, 6, 256):
            d_s, d_c = gpu_ctx.alloc((ngroups + 2) * 8), gpu_ctx.alloc((ngroups + 2) * 8)
            for words in (None, gpu_ctx.alloc(64).zero()):
                for d_counts in (d_c, None):
                    d_s.upload(np.full(ngroups + 2, POISON, dtype=np.uint64))
                    d_c.upload(np.full(ngroups + 2, POISON, dtype=np.uint64))
                    a.scan_group_sum_product(words, b, words, k, words, ngroups, d_s, d_counts)
                    assert d_s.download(np.uint64, ngroups + 2).tolist() == [0] * (ngroups + 1) + [POISON]
                    exp_c = [0] * (ngroups + 1) + [POISON] if d_counts is not None else [POISON] * (ngroups + 2)
                    assert d_c.download(np.uint64, ngroups + 2).tolist() == exp_c
