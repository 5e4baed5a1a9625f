"""adac_scan_group_sum_q1: COUNT, SUM(q), SUM(a), SUM(b), SUM(a * b), SUM(a * c), SUM(a * b * c) GROUP BY key over five
packed columns of one table in ONE scan, under a selection bitmap indexed in a's element space.

The expected value is numpy over the ORIGINAL columns (reference_q1): each of a, b, c and q widened to 64 bits by its own
signedness and viewed as uint64, multiplied and summed with dtype=uint64 (wraps mod 2^64, as the ABI says;
tests/test_group_sum_q1_abi.py holds it against Python integers), grouped by the key as an unsigned number of its own
width (keys >= ngroups in bin `ngroups`).  Compared exactly.  Where stated the seven terms are also held against the
existing entry points on the same encoded columns.  Every call is made twice into a buffer poisoned with 0xFF bytes
whose spare word after the 7 (ngroups + 1) results must stay poisoned.  Which kernel took what is read back after every
call (adac_debug_group_handover) and held against the host mirror of the rule (forms.group_q1_form_groups)."""
import importlib

import numpy as np
import pytest

from test_gpu_group_sum_product import INVALID_ARGUMENT, Col, NullLayout, widen
from test_gpu_group_sum_valid import dense_offsets, element_mask
from test_gpu_sum_product import kind_columns, segment_at_width

group_q1_form_groups = importlib.import_module("duckdb-adaptive-compression_amd.forms").group_q1_form_groups
pytestmark = pytest.mark.gpu

ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
FF = 0xFFFFFFFFFFFFFFFF
TERMS = 7
COUNT, SUM_Q, SUM_A, SUM_B, SUM_AB, SUM_AC, SUM_ABC = range(TERMS)


class q1_rw:
    """with q1_rw(adac, 0): the generic kernel alone; the default (1) restored on exit."""

    def __init__(self, adac, value):
        self.adac, self.value = adac, value

    def __enter__(self):
        self.adac.set_tuning("group_q1_rw", self.value)

    def __exit__(self, *exc):
        self.adac.set_tuning("group_q1_rw", 1)


def reference_q1(a, b, c, q, keys, ngroups, keep=None):
    """the seven terms, ngroups + 1 entries each: [COUNT, SUM(q), SUM(a), SUM(b), SUM(a b), SUM(a c), SUM(a b c)]"""
    x, y, z, v = widen(a), widen(b), widen(c), widen(q)
    ukeys = keys.view(np.dtype("u%d" % keys.dtype.itemsize)).astype(np.uint64)
    bins = np.minimum(ukeys, np.uint64(ngroups)).astype(np.int64)
    terms = [np.ones(len(x), dtype=np.uint64), v, x, y, x * y, x * z, x * y * z]
    if keep is not None:
        terms, bins = [t[keep] for t in terms], bins[keep]
    out = []
    for t in terms:
        acc = np.zeros(ngroups + 1, dtype=np.uint64)
        np.add.at(acc, bins, t)   # uint64: wraps mod 2^64
        out.append([int(s) for s in acc])
    return out


def kind(col):
    return col.vals.dtype.itemsize, col.vals.dtype.kind == "i"


class Encoded(Col):
    """a Col around a layout that was encoded elsewhere (another rule, padded widths, a re-encode)"""

    def __init__(self, vals, counts, lay, words):
        self.vals, self.counts, self.offs, self.lay, self.words = vals, counts, dense_offsets(counts), lay, words


class Quint:
    def __init__(self, ctx, a, b, c, q, k, ngroups):
        self.ctx, self.a, self.b, self.c, self.q, self.k, self.ngroups = ctx, a, b, c, q, k, ngroups
        self.span = int(a.lay.value_span)
        self.d_out = ctx.alloc((TERMS * (ngroups + 1) + 1) * 8)
        self._forms = None

    def forms(self):
        """{"fast": scan groups of a the register walk takes, "generic": the rest} by the host mirror of the rule"""
        if self._forms is None:
            self._forms = group_q1_form_groups(self.a.lay.get_descs(), self.b.lay.get_descs(), self.c.lay.get_descs(),
                                               self.q.lay.get_descs(), self.k.lay.get_descs(), self.ngroups,
                                               kind(self.a), kind(self.b), kind(self.c), kind(self.q),
                                               self.k.vals.dtype.itemsize)
        return self._forms

    def left_to_the_generic_kernel(self, rw=1):
        """what the register walk hands over, by the mirror; nothing when it is not launched (knob at 0, more than 8 bins)"""
        return self.forms()["generic"] if rw and self.ngroups + 1 <= 8 else 0

    def call(self, d_mask=None, rw=1):
        """the call, twice, each time into a poisoned buffer -> the seven terms; the hand-over word is the mirror's"""
        n = TERMS * (self.ngroups + 1)
        got = []
        for _ in range(2):
            self.d_out.upload(np.full(n + 1, FF, dtype=np.uint64))
            self.a.lay.scan_group_sum_q1(self.a.words, self.b.lay, self.b.words, self.c.lay, self.c.words, self.q.lay,
                                         self.q.words, self.k.lay, self.k.words, self.ngroups, self.d_out, d_mask)
            out = self.d_out.download(np.uint64, n + 1)
            assert int(out[n]) == FF   # nothing past the results
            assert self.a.lay.debug_group_handover() == self.left_to_the_generic_kernel(rw), ("hand-over", rw, self.forms())
            got.append(out[:n].reshape(TERMS, self.ngroups + 1).tolist())
        assert got[0] == got[1]
        return got[0]

    def upload_mask(self, keep, outside=False):
        return self.ctx.upload(element_mask(keep, self.a.counts, self.a.offs, self.span, outside))

    def expected(self, keep=None):
        return reference_q1(self.a.vals, self.b.vals, self.c.vals, self.q.vals, self.k.vals, self.ngroups, keep)

    def check(self, adac, keep, what, knobs=(1, 0), outside=False):
        """masked by `keep` (None: the NULL mask) against numpy, with the knob at each of `knobs`"""
        d_mask = None if keep is None else self.upload_mask(keep, outside)
        exp = self.expected(keep)
        assert sum(exp[COUNT]) == (len(self.a.vals) if keep is None else int(keep.sum()))
        for rw in knobs:
            with q1_rw(adac, rw):
                assert self.call(d_mask, rw) == exp, (what, "knob", rw)
        if d_mask is not None:
            d_mask.free()
        return exp


def six_calls(ctx, a, b, c, q, k, ngroups, d_mask):
    """the seven terms from the six existing calls on the same encoded columns"""
    d_s, d_c = ctx.alloc((ngroups + 1) * 8), ctx.alloc((ngroups + 1) * 8)
    n = ngroups + 1
    get = lambda d: d.download(np.uint64, n).tolist()
    q.lay.scan_group_sum_valid(q.words, k.lay, k.words, d_mask, ngroups, d_s, d_c)
    sum_q, cnt = get(d_s), get(d_c)
    a.lay.scan_group_sum_valid(a.words, k.lay, k.words, d_mask, ngroups, d_s, d_c)
    sum_a = get(d_s)
    assert get(d_c) == cnt
    b.lay.scan_group_sum_valid(b.words, k.lay, k.words, d_mask, ngroups, d_s, d_c)
    sum_b = get(d_s)
    assert get(d_c) == cnt
    a.lay.scan_group_sum_product(a.words, b.lay, b.words, k.lay, k.words, ngroups, d_s, None, d_mask)
    sum_ab = get(d_s)
    a.lay.scan_group_sum_product(a.words, c.lay, c.words, k.lay, k.words, ngroups, d_s, None, d_mask)
    sum_ac = get(d_s)
    a.lay.scan_group_sum_product3(a.words, b.lay, b.words, c.lay, c.words, k.lay, k.words, ngroups, d_s, None, d_mask)
    sum_abc = get(d_s)
    d_s.free()
    d_c.free()
    return [cnt, sum_q, sum_a, sum_b, sum_ab, sum_ac, sum_abc]


# ---------------------------------------------------------------------------------------------------------------------
# 1. Q1's shape; 8. the same under small and odd grids
# ---------------------------------------------------------------------------------------------------------------------
def q1_table(adac, ctx, n, seed):
    rng = np.random.default_rng(seed)
    counts = adac.appender_segment_counts(n, 4)
    code = rng.choice(6, size=n, p=[.2466, .2534, .0004, .2500, .2490, .0006]).astype(np.uint8)
    price = rng.integers(90_000, 10_495_000, size=n).astype(np.int32)
    qty = rng.integers(1, 51, size=n).astype(np.int32)
    disc = rng.integers(0, 11, size=n).astype(np.int32)
    tax = rng.integers(0, 9, size=n).astype(np.int32)
    date = rng.integers(8036, 10562, size=n).astype(np.int32)
    col = lambda v: Col(adac, ctx, v, counts)
    d, quint = col(date), Quint(ctx, col(price), col(disc), col(tax), col(qty), col(code), 6)
    cutoff = 10471
    d_bm = ctx.alloc((n + 63) // 64 * 8)
    d_sel = ctx.alloc(len(counts) * 8)
    int_min = int(np.array([np.iinfo(np.int32).min]).view(np.uint32)[0])
    d.lay.scan_select_between(d.words, int_min, cutoff, d_bm, d_sel)
    keep = date <= cutoff
    assert int(d_sel.download(np.uint64, len(counts)).sum()) == int(keep.sum()) and 0.8 * n < keep.sum() < n
    return quint, keep, d_bm


def test_q1_shape_against_numpy_and_the_six_calls(adac, gpu_ctx):
    t, keep, d_bm = q1_table(adac, gpu_ctx, 200_000, 1995)
    assert t.forms()["fast"] > 0 and t.forms()["generic"] == 0, t.forms()   # Q1's columns are the register walk's
    for d_mask, rows in ((d_bm, keep), (None, None)):
        exp = t.expected(rows)
        assert exp[COUNT][6] == 0 and all(exp[COUNT][:6])
        assert six_calls(gpu_ctx, t.a, t.b, t.c, t.q, t.k, 6, d_mask) == exp
        for rw in (1, 0, 1):
            with q1_rw(adac, rw):
                assert t.call(d_mask, rw) == exp, (rows is None, rw)
                assert t.a.lay.debug_group_handover() == 0   # knob 1: the fast form took every group; 0: not launched


@pytest.mark.parametrize("knob,value", [("num_cus", 1), ("num_cus", 2), ("num_cus", 3), ("num_cus", 32),
                                        ("scan_tiles_per_wg", 2), ("scan_tiles_per_wg", 16)])
def test_grid_sizes(adac, gpu_ctx, knob, value):
    t, keep, d_bm = q1_table(adac, gpu_ctx, 50_000, 8)
    try:
        adac.set_tuning(knob, value)
        for d_mask, rows in ((d_bm, keep), (None, None)):
            exp = t.expected(rows)
            for rw in (1, 0):
                with q1_rw(adac, rw):
                    assert t.call(d_mask, rw) == exp, (knob, value, rows is None, rw)
    finally:
        adac.set_tuning(knob, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fast form at every width of a, every staged width in every role, both forms of the keys
# ---------------------------------------------------------------------------------------------------------------------
STAGED_WIDTHS = (1, 4, 7, 13, 32)
ROWS2 = 1500


def column_of_widths(rng, dtype, widths, rows):
    """a segment of `rows` rows per entry of `widths`, packed at exactly that width: its first two rows are the ends of
    [base, base + 2^w) with base 1000 (0 at width 32: the whole of [0, 2^32))"""
    parts = []
    for w in widths:
        f = rng.integers(0, 2 ** w, size=rows, dtype=np.uint64)
        f[0], f[1] = 0, 2 ** w - 1
        parts.append(f + np.uint64(0 if w == 32 or np.dtype(dtype).itemsize == 1 else 1000))
    return np.concatenate(parts).astype(dtype)


def test_fast_form_at_every_width(adac, gpu_ctx):
    rng = np.random.default_rng(2)
    seg = [(i, j) for i in range(29) for j in range(5)]
    counts = np.full(len(seg), ROWS2, dtype=np.uint32)
    wa = [4 + i for i, j in seg]
    wb, wc, wq = ([STAGED_WIDTHS[(j + r) % 5] for i, j in seg] for r in (0, 1, 2))
    col = lambda widths, dtype=np.uint32: Col(adac, gpu_ctx, column_of_widths(rng, dtype, widths, ROWS2), counts)
    a, b, c, q = col(wa), col(wb), col(wc), col(wq)
    for made, want in ((a, wa), (b, wb), (c, wc), (q, wq)):
        assert made.widths() == want
    for r, widths in enumerate((wb, wc, wq)):   # every staged column meets every one of the five widths at every wa
        assert {(x, w) for x, w in zip(wa, widths)} == {(4 + i, w) for i in range(29) for w in STAGED_WIDTHS}, r
    n = int(counts.sum())
    keep = rng.random(n) < 0.5
    reached = set()
    # key widths 1 .. 8 cycle over the segments; the second cycle starts four further on, so that the five segments of
    # every width of a meet all eight between them: DIRECT keys (the keys of a chunk's rows fit a dword) and staged
    for start in (0, 4):
        wk = [1 + (s + start) % 8 for s in range(len(seg))]
        k = col(wk, np.uint8)
        assert k.widths() == wk
        t = Quint(gpu_ctx, a, b, c, q, k, 7)
        assert t.forms() == {"fast": len(seg), "generic": 0}, t.forms()   # one scan group per segment, all eligible
        reached |= {(x, (128 + x - 1) // x * w <= 32) for x, w in zip(wa, wk)}
        t.check(adac, keep, ("masked", start), knobs=(1,))
        t.check(adac, None, ("NULL mask", start), knobs=(1, 0) if start == 0 else (1,))
        assert t.a.lay.debug_group_handover() == 0
    # the keys of a 32-bit chunk row (four rows) always fit a dword: no staged form there; everything else is reached
    assert reached == {(x, direct) for x in range(4, 33) for direct in (True, False)} - {(32, False)}


# ---------------------------------------------------------------------------------------------------------------------
# 3. the generic form: every type in every role, widths up to the type's, every segment kind, up to 257 bins
# ---------------------------------------------------------------------------------------------------------------------
COUNTS3 = np.array([0, 1, 31, 64, 2047, 2048, 2049, 4097, 32767, 65534, 70001], dtype=np.uint32)
ROLE_SHIFTS = (0, 3, 5, 6)   # a, b, c, q: assignment t gives role r the type ALL[(t + shift) % 8]
NGROUPS3 = (1, 7, 8, 200, 256)


def random_width_column(rng, dtype, counts):
    dtype = np.dtype(dtype)
    parts = [segment_at_width(rng, dtype, int(c), int(rng.integers(1, 8 * dtype.itemsize + 1))) if c else
             np.zeros(0, dtype=dtype) for c in counts]
    return np.concatenate(parts)


def test_role_shifts_put_every_type_in_every_role_once():
    for shift in ROLE_SHIFTS:
        assert sorted((t + shift) % 8 for t in range(8)) == list(range(8))


@pytest.fixture(scope="module")
def generic_shared(adac, gpu_ctx):
    """one column per type at random widths (shared by the roles and the assignments), the keys and the mask"""
    rng = np.random.default_rng(3)
    n = int(COUNTS3.sum())
    cols = {np.dtype(t).name: Col(adac, gpu_ctx, random_width_column(rng, t, COUNTS3), COUNTS3) for t in ALL}
    assert any(w > 32 for w in cols["uint64"].widths()) and any(w > 32 for w in cols["int64"].widths())
    assert (cols["int32"].vals < 0).any() and (cols["int8"].vals < 0).any()
    keys = Col(adac, gpu_ctx, rng.integers(0, 300, size=n).astype(np.uint16), COUNTS3)   # below and at or above every ngroups
    return cols, keys, rng.random(n) < 0.5


@pytest.mark.parametrize("assignment", range(8))
def test_generic_form_every_type_in_every_role(adac, gpu_ctx, generic_shared, assignment):
    cols, keys, keep = generic_shared
    a, b, c, q = (cols[np.dtype(ALL[(assignment + s) % 8]).name] for s in ROLE_SHIFTS)
    for ngroups in NGROUPS3:
        t = Quint(gpu_ctx, a, b, c, q, keys, ngroups)
        exp = t.check(adac, keep, (assignment, ngroups, "half"), knobs=(1,))
        assert exp[COUNT][ngroups] > 0 and (ngroups == 1 or min(exp[COUNT][:ngroups]) > 0)   # keys on both sides of ngroups
        t.check(adac, None, (assignment, ngroups, "NULL mask"), knobs=(1,) if ngroups != 7 else (1, 0))


def test_generic_form_segment_kinds_in_every_role(adac, gpu_ctx):
    """unpacked segments, a range that wraps the sign boundary under the recompact rule, the all-ones stored min of an
    all -1 int64 column, padding to bytes: each kind in each of the four value roles"""
    from test_gpu_sum_product import COUNTS3 as counts
    from test_gpu_sum_product import encode_column
    rng = np.random.default_rng(33)
    n = int(counts.sum())
    enc = []
    for name, (vals, rule, pad, check) in kind_columns().items():
        col = Encoded(vals, counts, *encode_column(adac, gpu_ctx, vals, counts, rule=rule, pad=pad))
        assert check(col.lay.get_descs()), name
        enc.append(col)
    keys = Col(adac, gpu_ctx, rng.integers(0, 10, size=n).astype(np.uint8), counts)
    keep = rng.random(n) < 0.5
    for i in range(len(enc)):
        a, b, c, q = (enc[(i + r) % len(enc)] for r in (0, 1, 2, 3))
        for ngroups in (7, 200):
            t = Quint(gpu_ctx, a, b, c, q, keys, ngroups)
            t.check(adac, keep, (i, ngroups, "half"), knobs=(1, 0) if ngroups == 7 else (1,))
            t.check(adac, None, (i, ngroups, "NULL mask"), knobs=(1,))


# ---------------------------------------------------------------------------------------------------------------------
# 4. both forms in one call
# ---------------------------------------------------------------------------------------------------------------------
def test_mixed_forms_in_one_call(adac, gpu_ctx):
    """segments alternate between an eligible quintuple and one the walk must leave: `a` at width 40, c signed with
    negative values, keys at 9 bits (in turn)"""
    rng = np.random.default_rng(4)
    counts = np.array([3000, 2049, 70001, 1, 4097, 65534, 333, 2048, 5000, 31, 20000, 64], dtype=np.uint32)
    a, c, k = [], [], []
    for s, n in enumerate(int(x) for x in counts):
        why = (None, "a", None, "c", None, "k")[s % 6]
        f = rng.integers(0, 2 ** 40 if why == "a" else 2 ** 20, size=n, dtype=np.uint64)
        if n >= 2:
            f[0], f[1] = 0, (2 ** 40 if why == "a" else 2 ** 20) - 1
        a.append(f + np.uint64(1000))
        c.append(rng.integers(-20, 21, size=n) if why == "c" else rng.integers(0, 9, size=n))
        if why == "c" and n >= 1:
            c[-1][0] = -20
        kk = rng.integers(0, 6, size=n)
        if why == "k" and n >= 2:
            kk[0], kk[1] = 0, 511   # nine bits
        k.append(kk)
    n = int(counts.sum())
    col = lambda parts, dtype: Col(adac, gpu_ctx, np.concatenate(parts).astype(dtype), counts)
    t = Quint(gpu_ctx, col(a, np.uint64), Col(adac, gpu_ctx, rng.integers(0, 11, size=n).astype(np.uint8), counts),
              col(c, np.int32), Col(adac, gpu_ctx, rng.integers(1, 51, size=n).astype(np.int16), counts),
              col(k, np.uint16), 6)
    assert [w for s, w in enumerate(t.a.widths()) if s % 6 == 1 and counts[s] >= 2] == [40, 40]
    assert [w for s, w in enumerate(t.k.widths()) if s % 6 == 5 and counts[s] >= 2] == [9, 9]
    # segment by segment: the walk takes the even ones whole and none of the odd ones
    descs = [x.lay.get_descs() for x in (t.a, t.b, t.c, t.q, t.k)]
    per_seg = [group_q1_form_groups(*([d[s]] for d in descs), 6, kind(t.a), kind(t.b), kind(t.c), kind(t.q), 2)
               for s in range(len(counts))]
    for s, f in enumerate(per_seg):
        assert (f["generic"] == 0 and f["fast"] > 0) if s % 2 == 0 else (f["fast"] == 0 and f["generic"] > 0), (s, f)
    assert t.forms()["generic"] == sum(f["generic"] for f in per_seg) > 0
    for name, keep in (("half", rng.random(n) < 0.5), ("NULL mask", None)):
        t.check(adac, keep, name, knobs=(1, 0, 1))   # call() holds the hand-over word to the mirror's count


# ---------------------------------------------------------------------------------------------------------------------
# 5. the mask is indexed in a's element space
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("types,bits", [((np.int32, np.uint16, np.int8, np.uint8), (21, 9, 5, 6)),
                                        ((np.int64, np.int8, np.uint32, np.int16), (40, 5, 30, 11))])
def test_mask_in_a_element_space(adac, gpu_ctx, types, bits):
    rng = np.random.default_rng(5 + bits[0])
    counts = np.array([1, 70, 2048, 9000, 0, 333, 4097, 64, 31, 20000] * 2, dtype=np.uint32)
    n = int(counts.sum())
    gaps = lambda: np.cumsum(rng.integers(0, 71, size=len(counts)) + np.concatenate([[0], counts[:-1]])).astype(np.uint64)
    offs = [gaps() for _ in range(5)]   # a, b, c, q, keys: five layouts with different gaps between the segments
    assert all((x != y).any() for i, x in enumerate(offs) for y in offs[i + 1:])
    assert len({int(o) & 63 for o in offs[0]}) > 10   # segments start at many bit phases of a mask word
    vals = [np.concatenate([segment_at_width(rng, ty, int(c), w) if c else np.zeros(0, dtype=ty) for c in counts])
            for ty, w in zip(types, bits)]
    cols = [Col(adac, gpu_ctx, v, counts, o) for v, o in zip(vals, offs)]
    keys = Col(adac, gpu_ctx, rng.integers(0, 9, size=n).astype(np.uint8), counts, offs[4])
    t = Quint(gpu_ctx, *cols, keys, 7)
    ends = np.zeros(n, dtype=bool)
    ends[dense_offsets(counts).astype(np.int64)[counts > 0]] = True
    ends[(np.cumsum(counts) - 1)[counts > 0]] = True
    masks = {"ones": np.ones(n, dtype=bool), "zeros": np.zeros(n, dtype=bool), "half": rng.random(n) < 0.5,
             "one percent": rng.random(n) < 0.01, "first and last rows": ends}
    t.check(adac, None, "NULL mask")
    for name, keep in masks.items():
        exp = t.check(adac, keep, name)
        t.check(adac, keep, (name, "bits of no row set"), knobs=(1,), outside=True)
        if name == "zeros":
            assert not any(any(row) for row in exp)
        if name == "ones":
            assert exp == t.expected()
    # the same rows kept, but the mask laid out in b's element space: a different answer, so the space used is a's
    keep = masks["half"]
    span = max(t.span, int(t.b.lay.value_span))
    d_mask = gpu_ctx.upload(element_mask(keep, counts, offs[1], span))
    assert t.call(d_mask) != t.expected(keep)
    d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 6. aliasing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,bits", [(np.uint32, 19), (np.int16, 11)])
def test_one_column_in_all_four_roles(adac, gpu_ctx, dtype, bits):
    rng = np.random.default_rng(6)
    counts = np.array([70001, 333, 0, 4097], dtype=np.uint32)
    n = int(counts.sum())
    x = np.concatenate([segment_at_width(rng, dtype, int(c), bits) if c else np.zeros(0, dtype=dtype) for c in counts])
    a = Col(adac, gpu_ctx, x, counts)
    assert [w for w, cnt in zip(a.widths(), counts) if cnt] == [bits] * 3
    k = Col(adac, gpu_ctx, rng.integers(0, 6, size=n).astype(np.uint8), counts)
    t = Quint(gpu_ctx, a, a, a, a, k, 6)
    keep = rng.random(n) < 0.3
    for rows in (None, keep):
        exp = t.check(adac, rows, "a == b == c == q")
        sel = np.ones(n, dtype=bool) if rows is None else rows
        for g in range(7):
            vs = [int(v) for v in x[sel & (np.minimum(k.vals, 6) == g)]]
            s1, s2, s3 = (sum(v ** p for v in vs) % 2 ** 64 for p in (1, 2, 3))
            assert [exp[i][g] for i in range(TERMS)] == [len(vs), s1, s1, s1, s2, s2, s3], g


# ---------------------------------------------------------------------------------------------------------------------
# 7. interleaved with the other grouped scans; across re-encodes of a; layouts without rows
# ---------------------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_grouped_scans_and_across_reencodes(adac, gpu_ctx):
    rng = np.random.default_rng(7)
    counts = np.array([30000, 2049, 1, 65534, 4097], dtype=np.uint32)
    n = int(counts.sum())
    mk = lambda lo, hi, dtype: Col(adac, gpu_ctx, rng.integers(lo, hi, size=n).astype(dtype), counts)
    a, b, c, q, k = mk(1000, 1000 + 2 ** 13, np.int32), mk(0, 11, np.uint8), mk(-3, 9, np.int16), mk(1, 51, np.uint32), \
        mk(0, 8, np.uint8)
    t = Quint(gpu_ctx, a, b, c, q, k, 6)
    keep = rng.random(n) < 0.5
    d_mask = t.upload_mask(keep)
    exp, exp_all = t.expected(keep), t.expected()
    d_s, d_c = gpu_ctx.alloc(8 * 8), gpu_ctx.alloc(8 * 8)

    def pair(with_counts=True):
        s, cnt = d_s.download(np.uint64, 8).tolist(), d_c.download(np.uint64, 8).tolist()
        assert s[7] == FF and cnt[7] == FF
        return (s[:7], cnt[:7]) if with_counts else s[:7]

    def poison():
        d_s.upload(np.full(8, FF, dtype=np.uint64))
        d_c.upload(np.full(8, FF, dtype=np.uint64))

    def other(which):
        for _ in range(2):
            poison()
            if which == "s":     # adac_scan_group_sum: every row
                a.lay.scan_group_sum(a.words, k.lay, k.words, 6, d_s, d_c)
                assert pair() == (exp_all[SUM_A], exp_all[COUNT])
            elif which == "v":
                a.lay.scan_group_sum_valid(a.words, k.lay, k.words, d_mask, 6, d_s, d_c)
                assert pair() == (exp[SUM_A], exp[COUNT])
            elif which == "p":
                a.lay.scan_group_sum_product(a.words, c.lay, c.words, k.lay, k.words, 6, d_s, d_c, d_mask)
                assert pair() == (exp[SUM_AC], exp[COUNT])
            else:
                a.lay.scan_group_sum_product3(a.words, b.lay, b.words, c.lay, c.words, k.lay, k.words, 6, d_s, d_c, d_mask)
                assert pair() == (exp[SUM_ABC], exp[COUNT])

    order = list("1s1vp13v11ps3v1p3s11")   # fixed: a shuffle of the fused call (1) and the four existing entry points
    assert len(order) == 20 and set(order) == set("1svp3")
    for rw in (1, 0):
        with q1_rw(adac, rw):
            for i, which in enumerate(order):
                if which == "1":
                    assert t.call(d_mask if i % 3 else None, rw) == (exp if i % 3 else exp_all), (rw, i)
                else:
                    other(which)
    # `a` re-encoded into the layout the fused call reads: padded widths first, then the tight ones again
    lay = adac.Layout(gpu_ctx, np.int32, counts)
    dst = Encoded(a.vals, counts, lay, gpu_ctx.alloc(lay.max_arena_words * 8 + 16).zero())
    t2 = Quint(gpu_ctx, dst, b, c, q, k, 6)
    for pad, width in ((True, 16), (False, 13), (True, 16)):
        a.lay.reencode(a.words, dst.lay, dst.words, pad_to_byte=pad)
        assert {w for w, cnt in zip(dst.widths(), counts) if cnt > 1} == {width}, dst.widths()
        t2._forms = None
        assert t2.call(d_mask) == exp and t2.call(None) == exp_all, pad
    d_mask.free()


def test_layouts_without_rows_write_zeros(adac, gpu_ctx):
    for counts in (np.array([0, 0, 0], dtype=np.uint32), np.array([0], dtype=np.uint32)):
        lays = [adac.Layout(gpu_ctx, t, counts) for t in (np.int32, np.uint8, np.int64, np.uint16, np.uint8)]
        a, b, c, q, k = lays
        for ngroups in (1, 6, 256):
            n = TERMS * (ngroups + 1)
            d_out = gpu_ctx.alloc((n + 1) * 8)
            for words in (None, gpu_ctx.alloc(64).zero()):
                for _ in range(2):
                    d_out.upload(np.full(n + 1, FF, dtype=np.uint64))
                    a.scan_group_sum_q1(words, b, words, c, words, q, words, k, words, ngroups, d_out)
                    assert d_out.download(np.uint64, n + 1).tolist() == [0] * n + [FF]
                    assert a.debug_group_handover() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_codec_usable(adac, gpu_ctx):
    rng = np.random.default_rng(9)
    counts = np.array([100, 3000], dtype=np.uint32)
    n = int(counts.sum())
    mk = lambda hi, dtype: Col(adac, gpu_ctx, rng.integers(0, hi, size=n).astype(dtype), counts)
    t = Quint(gpu_ctx, mk(2 ** 17, np.uint32), mk(11, np.int16), mk(9, np.int32), mk(51, np.uint8), mk(5, np.uint8), 4)
    a, b, c, q, k = (x.lay for x in (t.a, t.b, t.c, t.q, t.k))
    wa, wb, wc, wq, wk = (x.words for x in (t.a, t.b, t.c, t.q, t.k))
    other = adac.Layout(gpu_ctx, np.uint8, np.array([100, 3001], dtype=np.uint32))
    d = gpu_ctx.alloc(4096)
    d.upload(np.full(512, FF, dtype=np.uint64))
    good = [a, wa, b, wb, c, wc, q, wq, k, wk, 4, d]
    ctx2 = adac.Context(0)
    try:
        far = adac.Layout(ctx2, np.uint8, counts)

        def with_(changes):
            args = list(good)
            for i, v in changes.items():
                args[i] = v
            return lambda: adac.Layout.scan_group_sum_q1(*args)

        refused = {}
        for i, role in ((0, "a"), (2, "b"), (4, "c"), (6, "q"), (8, "keys")):
            refused["NULL " + role] = with_({i: NullLayout})
            refused[role + " on another context"] = with_({i: far})
            refused["counts of " + role] = with_({i: other})
            refused["NULL words of " + role] = with_({i + 1: None})
            refused["words of %s off by 8" % role] = with_({i + 1: good[i + 1].ptr + 8})
        refused["ngroups 0"] = with_({10: 0})
        refused["ngroups 257"] = with_({10: 257})
        refused["NULL d_out"] = with_({11: None})
        for what, call in refused.items():
            with pytest.raises(adac.AdacError) as e:
                call()
            assert e.value.status == INVALID_ARGUMENT, what
        assert d.download(np.uint64, 512).tolist() == [FF] * 512   # refused before any launch: nothing was written
        far.close()
    finally:
        ctx2.close()
    assert t.call(None) == t.expected()   # a correct call afterwards
