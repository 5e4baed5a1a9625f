"""adac_scan_group_sum_valid: SUM(value), COUNT(*) GROUP BY key over two packed columns, restricted to the rows whose bit
is set in a selection / validity bitmap indexed in the VALUE layout's element space (val_off + row) — Q1 with its WHERE
clause.  The reference has no grouped scan (its engine aggregates decoded vectors); parity, as for the unmasked call
(tests/test_gpu_group_sum.py), is numpy's GROUP BY over the kept rows of the raw columns, compared exactly mod 2^64:
reference_groups(vals[m], keys[m], ngroups) with m read from the mask at val_off + row.

Both kernel forms are held to it: the register walk (k_group_sum_rw<true>) and the staged-LDS kernel (k_group_sum<true>,
alone under group_sum_rw = 0, and for the segment pairs the walk leaves).  Results are poisoned before every call.
Element indices past 2^32 are not reached here (the value buffer alone would take tens of GB)."""
import numpy as np
import pytest

from test_gpu_grid_sizes import knobs
from test_gpu_group_sum import encode_column, reference_groups
from test_gpu_group_sum_rw import every_width_column, mixed_walk_column

pytestmark = pytest.mark.gpu

ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
POISON = 0xDEADBEEFDEADBEEF


def dense_offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)


def element_mask(keep, counts, offs, span, outside=False):
    """bool per row -> exactly ceil(span / 64) u64 words over the element space in which segment i starts at offs[i];
    every bit that belongs to no row (gaps, the tail of the last word) is `outside`."""
    nwords = max((int(span) + 63) // 64, 1)
    full = np.full(nwords * 64, outside, dtype=bool)
    pos = 0
    for c, o in zip(counts, offs):
        full[int(o):int(o) + int(c)] = keep[pos:pos + int(c)]
        pos += int(c)
    return np.packbits(full, bitorder="little").view(np.uint64)


def clustered(rng, n):
    """Runs of kept and dropped rows, 130 .. 500 rows each (so whole all-ones and whole zero words lie inside) whose
    ends never fall on a multiple of 64."""
    keep = np.zeros(n, dtype=bool)
    pos, on = 0, True
    while pos < n:
        run = int(rng.integers(130, 500))
        if (pos + run) % 64 == 0:
            run += 1
        keep[pos:pos + run] = on
        pos += run
        on = not on
    return keep


def mask_shapes(rng, counts):
    n = int(counts.sum())
    live = counts > 0
    first = dense_offsets(counts).astype(np.int64)[live]
    last = (np.cumsum(counts).astype(np.int64) - 1)[live]
    shapes = {"ones": np.ones(n, dtype=bool), "zeros": np.zeros(n, dtype=bool), "half": rng.random(n) < 0.5,
              "first rows": np.zeros(n, dtype=bool), "last rows": np.zeros(n, dtype=bool), "clustered": clustered(rng, n)}
    shapes["first rows"][first] = True
    shapes["last rows"][last] = True
    return shapes


def make_case(rng, vdtype, kdtype, n, vbits, key_top):
    """The columns of test_gpu_group_sum.run_case: values in a vbits-wide range at a random base, keys below key_top."""
    vdtype, kdtype = np.dtype(vdtype), np.dtype(kdtype)
    tb = 8 * vdtype.itemsize
    span = rng.integers(0, 2 ** min(vbits, tb), size=n, dtype=np.uint64)
    base = int(rng.integers(0, 2 ** tb - 2 ** min(vbits, tb) + 1, dtype=np.uint64)) if vbits < tb else 0
    vals = ((span + np.uint64(base)) & np.uint64(2 ** tb - 1)).astype(np.dtype("u%d" % vdtype.itemsize)).view(vdtype)
    keys = rng.integers(0, key_top, size=n, dtype=np.uint64).astype(np.dtype("u%d" % kdtype.itemsize)).view(kdtype)
    return vals, keys


class Pair:
    """A value and a key column encoded on the same rows, and the two result buffers."""

    def __init__(self, adac, ctx, vals, keys, counts, ngroups, voffs=None, koffs=None):
        self.ctx, self.vals, self.keys, self.counts, self.ngroups = ctx, vals, keys, counts, ngroups
        self.voffs = dense_offsets(counts) if voffs is None else voffs
        self.vlay, self.vwords = encode_column(adac, ctx, vals, counts, voffs)
        self.klay, self.kwords = encode_column(adac, ctx, keys, counts, koffs)
        self.span = int(self.vlay.value_span)
        self.d_sums, self.d_cnts = ctx.alloc((ngroups + 1) * 8), ctx.alloc((ngroups + 1) * 8)

    def poison(self):
        self.d_sums.upload(np.full(self.ngroups + 1, POISON, dtype=np.uint64))
        self.d_cnts.upload(np.full(self.ngroups + 1, POISON, dtype=np.uint64))

    def results(self):
        n = self.ngroups + 1
        return self.d_sums.download(np.uint64, n).tolist(), self.d_cnts.download(np.uint64, n).tolist()

    def masked(self, d_mask):
        self.poison()
        self.vlay.scan_group_sum_valid(self.vwords, self.klay, self.kwords, d_mask, self.ngroups, self.d_sums, self.d_cnts)
        return self.results()

    def plain(self):
        self.poison()
        self.vlay.scan_group_sum(self.vwords, self.klay, self.kwords, self.ngroups, self.d_sums, self.d_cnts)
        return self.results()

    def upload_mask(self, keep, outside=False):
        return self.ctx.upload(element_mask(keep, self.counts, self.voffs, self.span, outside))

    def expected(self, keep=None):
        if keep is None:
            return tuple(reference_groups(self.vals, self.keys, self.ngroups))
        return tuple(reference_groups(self.vals[keep], self.keys[keep], self.ngroups))

    def check(self, keep, what, outside=False):
        """One masked call against numpy; the counts add up to the kept rows."""
        d_mask = self.upload_mask(keep, outside)
        got = self.masked(d_mask)
        d_mask.free()
        assert got == self.expected(keep), what
        assert sum(got[1]) == int(keep.sum()), what
        return got

    def check_three_ways(self, adac, keep, what):
        """The register walk, the staged kernel alone, the register walk again (the hand-over word was left at zero)."""
        d_mask = self.upload_mask(keep)
        exp = self.expected(keep)
        for rw in (1, 0, 1):
            with knobs(adac, group_sum_rw=rw):
                assert self.masked(d_mask) == exp, (what, rw)
        d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 1. every value type, three key shapes, six mask shapes; 6. NULL mask == the old entry point on the same columns
# ---------------------------------------------------------------------------------------------------------------------
COUNTS1 = np.array([2048, 32767, 1, 0, 5000, 70001, 63, 4096], dtype=np.uint32)
KEY_CASES = ((np.uint8, 6, 6), (np.uint16, 40, 50), (np.int32, 256, 300))


def type_cases(adac, ctx, vdtype):
    vdtype = np.dtype(vdtype)
    rng = np.random.default_rng(770 + vdtype.itemsize + (vdtype.kind == "i"))
    tb = 8 * vdtype.itemsize
    for kdtype, ngroups, key_top in KEY_CASES:
        for vbits in (6, tb // 2 + 1):
            vals, keys = make_case(rng, vdtype, kdtype, int(COUNTS1.sum()), vbits, key_top)
            yield (np.dtype(kdtype).name, ngroups, vbits), Pair(adac, ctx, vals, keys, COUNTS1, ngroups)


@pytest.mark.parametrize("vdtype", ALL)
def test_every_value_type_under_every_mask_shape(adac, gpu_ctx, vdtype):
    shapes = mask_shapes(np.random.default_rng(11), COUNTS1)
    assert shapes["first rows"].sum() == shapes["last rows"].sum() == 7 and 0.4 < shapes["clustered"].mean() < 0.6
    for case, pair in type_cases(adac, gpu_ctx, vdtype):
        for name, keep in shapes.items():
            got = pair.check(keep, (case, name))
            if name == "zeros":
                assert not any(got[0]) and not any(got[1])
            if name == "ones":
                assert got == pair.expected()


@pytest.mark.parametrize("vdtype", ALL)
def test_null_mask_is_the_unmasked_call(adac, gpu_ctx, vdtype):
    for case, pair in type_cases(adac, gpu_ctx, vdtype):
        a, b = pair.masked(None), pair.plain()
        assert a == b == pair.expected(), case


# ---------------------------------------------------------------------------------------------------------------------
# 2. both kernel forms at every walk width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", [np.uint32, np.int32, np.uint64, np.uint16])
def test_both_kernel_forms_at_every_walk_width(adac, gpu_ctx, vdtype):
    vdtype = np.dtype(vdtype)
    rng = np.random.default_rng(310 + vdtype.itemsize)
    widths, counts, vals = every_width_column(rng, vdtype)
    masks = {"half": rng.random(len(vals)) < 0.5, "clustered": clustered(rng, len(vals))}
    for wk in (1, 3, 5, 8):
        keys = rng.integers(0, 2 ** wk, size=len(vals)).astype(np.uint8)
        pair = Pair(adac, gpu_ctx, vals, keys, counts, 7)
        assert sorted(set(pair.vlay.get_descs()["width"].tolist())) == widths
        assert set(pair.klay.get_descs()["width"].tolist()) <= {wk, wk + 1}
        for name, keep in masks.items():
            pair.check_three_ways(adac, keep, (wk, name))


def test_segments_the_walk_leaves_go_through_the_staged_kernel_under_the_mask(adac, gpu_ctx):
    rng = np.random.default_rng(5150)
    vals, keys, counts = mixed_walk_column(rng)
    pair = Pair(adac, gpu_ctx, vals, keys, counts, 6)
    assert pair.vlay.get_descs()["width"].tolist()[:5] == [2, 40, 13, 1, 24]
    masks = {"half": rng.random(len(vals)) < 0.5, "clustered": clustered(rng, len(vals))}
    for name, keep in masks.items():
        pair.check_three_ways(adac, keep, name)
    for wide in (0, 1):   # the staged kernel's 32-bit and 64-bit row loops
        with knobs(adac, group_sum_wide=wide):
            pair.check_three_ways(adac, masks["half"], ("wide", wide))
    unsigned = Pair(adac, gpu_ctx, (vals & 0x7fffffff).astype(np.uint32), keys.astype(np.uint8), counts, 3)
    for wide in (0, 1):
        with knobs(adac, group_sum_wide=wide):
            unsigned.check_three_ways(adac, masks["clustered"], ("uint32 wide", wide))


# ---------------------------------------------------------------------------------------------------------------------
# 3. every phase of a segment's first bit in its mask word; 4. bits that belong to no row
# ---------------------------------------------------------------------------------------------------------------------
def phase_column(rng):
    """64 uint32 segments, segment i at an element offset with val_off & 63 == i (gaps between them); the key layout
    has other offsets.  Values at width 13, keys at width 3 (key 7 lands in the overflow bin of 7 groups).  The last
    segment ends inside a mask word, so that word has a tail that belongs to no row."""
    counts = np.array([(1, 63, 64, 65, 129, 4097 + i)[(i + 2) % 6] for i in range(64)], dtype=np.uint32)
    voffs, run = [], 0
    for i, c in enumerate(counts):
        run += 64 if run % 64 == i else 0          # never back to back
        run += (i - run) % 64
        voffs.append(run)
        run += int(c)
    voffs = np.array(voffs, dtype=np.uint64)
    koffs = np.cumsum(np.concatenate([[1], counts[:-1] + 2 * np.arange(1, 64)])).astype(np.uint64)
    n = int(counts.sum())
    vals = (rng.integers(0, 2 ** 13, size=n) + 100_000).astype(np.uint32)
    for s, c in zip(dense_offsets(counts).astype(np.int64), counts):
        if c >= 2:
            vals[s], vals[s + 1] = 100_000, 100_000 + 2 ** 13 - 1
    keys = rng.integers(0, 8, size=n).astype(np.uint8)
    return vals, keys, counts, voffs, koffs


def test_every_mask_phase(adac, gpu_ctx):
    rng = np.random.default_rng(63)
    vals, keys, counts, voffs, koffs = phase_column(rng)
    assert [int(o) & 63 for o in voffs] == list(range(64)) and (voffs != koffs).any()
    assert all(int(voffs[i]) + int(counts[i]) < int(voffs[i + 1]) for i in range(63))
    pair = Pair(adac, gpu_ctx, vals, keys, counts, 7, voffs, koffs)
    widths = pair.vlay.get_descs()["width"][counts >= 2].tolist()
    assert set(widths) == {13} and set(pair.klay.get_descs()["width"][counts >= 63].tolist()) == {3}
    for seed in range(3):
        keep = np.random.default_rng(seed).random(len(vals)) < 0.5
        pair.check_three_ways(adac, keep, seed)
    pair.check_three_ways(adac, np.ones(len(vals), dtype=bool), "ones")


@pytest.mark.parametrize("vdtype,kdtype,ngroups,vbits,key_top", [(np.int32, np.uint8, 4, 21, 4),
                                                                 (np.int64, np.int16, 200, 33, 200)])
def test_gapped_layouts(adac, gpu_ctx, vdtype, kdtype, ngroups, vbits, key_top):
    """run_case's gaps=True placement: the two columns sit at different element offsets; the mask follows the values'."""
    rng = np.random.default_rng(99)
    counts = np.array([1000, 37, 5000, 2048, 1, 16385], dtype=np.uint32)
    voffs = np.cumsum(np.concatenate([[3], counts[:-1] + 5]).astype(np.uint64))
    koffs = np.cumsum(np.concatenate([[1], counts[:-1] + 2]).astype(np.uint64))
    vals, keys = make_case(rng, vdtype, kdtype, int(counts.sum()), vbits, key_top)
    pair = Pair(adac, gpu_ctx, vals, keys, counts, ngroups, voffs, koffs)
    for name, keep in mask_shapes(rng, counts).items():
        pair.check_three_ways(adac, keep, name)
        pair.check(keep, (name, "gap bits set"), outside=True)


def test_bits_outside_the_segments_never_matter(adac, gpu_ctx):
    """The mask is a 16-byte-aligned slice inside a larger buffer.  Once every bit that belongs to no row is clear —
    gaps, the tail of the last word, two sentinel words on either side — and once all of them are set."""
    rng = np.random.default_rng(64)
    vals, keys, counts, voffs, koffs = phase_column(rng)
    pair = Pair(adac, gpu_ctx, vals, keys, counts, 7, voffs, koffs)
    assert pair.span % 64 != 0   # the last word has a tail
    keep = rng.random(len(vals)) < 0.5
    exp = pair.expected(keep)
    got = {}
    for outside in (False, True):
        words = element_mask(keep, counts, voffs, pair.span, outside)
        assert len(words) == (pair.span + 63) // 64
        sentinel = np.full(2, 0xFFFFFFFFFFFFFFFF if outside else 0, dtype=np.uint64)
        d_big = gpu_ctx.upload(np.concatenate([sentinel, words, sentinel]))
        for rw in (1, 0):
            with knobs(adac, group_sum_rw=rw):
                got[outside, rw] = pair.masked(d_big.ptr + 16)
        d_big.free()
    assert all(g == exp for g in got.values()), [k for k, g in got.items() if g != exp]


# ---------------------------------------------------------------------------------------------------------------------
# 5. chained after the filter
# ---------------------------------------------------------------------------------------------------------------------
def test_chained_after_the_filter(adac, gpu_ctx):
    """Q1's shape at 1 M rows: the bitmap adac_scan_select_between writes for l_shipdate <= cutoff is handed, as the same
    device buffer, to the grouped scan of both value columns; then the same with 10 % NULL rows given to the select."""
    rng = np.random.default_rng(1998)
    n = 1_000_000
    counts = np.array([65534] * (n // 65534) + [n % 65534], dtype=np.uint32)
    code = rng.choice(6, size=n, p=[.25, .25, .01, .24, .24, .01]).astype(np.uint8)
    cols = {"l_quantity": rng.integers(1, 51, size=n, dtype=np.int64).astype(np.int32),
            "l_partkey": rng.integers(1, 2_000_001, size=n, dtype=np.int64).astype(np.int32)}
    date = rng.integers(8036, 10562, size=n).astype(np.int32)
    cutoff = 10471
    dlay, dwords = encode_column(adac, gpu_ctx, date, counts)
    pairs = {name: Pair(adac, gpu_ctx, v, code, counts, 6) for name, v in cols.items()}
    d_bm = gpu_ctx.alloc((n + 63) // 64 * 8)
    d_sel = gpu_ctx.alloc(len(counts) * 8)
    int_min = int(np.array([np.iinfo(np.int32).min]).view(np.uint32)[0])
    valid = rng.random(n) >= 0.1
    d_valid = gpu_ctx.upload(element_mask(valid, counts, dense_offsets(counts), n))
    for d_validity, rows in ((None, np.ones(n, dtype=bool)), (d_valid, valid)):
        dlay.scan_select_between(dwords, int_min, cutoff, d_bm, d_sel, d_validity)
        selected = int(d_sel.download(np.uint64, len(counts)).sum())
        m = (date <= cutoff) & rows
        assert selected == int(m.sum()) and 0.8 * n < selected < n
        for name, pair in pairs.items():
            got = pair.masked(d_bm)
            assert got == pair.expected(m), name
            assert sum(got[1]) == selected and got[1][6] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. other grid sizes, masked and unmasked calls in turn on the same layouts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [1, 3])
def test_small_grids_and_alternating_calls(adac, gpu_ctx, cus):
    rng = np.random.default_rng(7 + cus)
    widths, counts, vals = every_width_column(rng, np.dtype(np.uint32))
    every = Pair(adac, gpu_ctx, vals, rng.integers(0, 8, size=len(vals)).astype(np.uint8), counts, 7)
    mvals, mkeys, mcounts = mixed_walk_column(rng)
    mixed = Pair(adac, gpu_ctx, mvals, mkeys, mcounts, 6)
    for pair in (every, mixed):
        keep = rng.random(len(pair.vals)) < 0.5
        d_mask = pair.upload_mask(keep)
        exp_masked, exp_plain = pair.expected(keep), pair.expected()
        with knobs(adac, num_cus=cus):
            for rw in (1, 0, 1):
                with knobs(adac, group_sum_rw=rw):
                    for rep in range(2):   # the two-slot hand-over word survives the alternation
                        assert pair.masked(d_mask) == exp_masked, (cus, rw, rep)
                        assert pair.plain() == exp_plain, (cus, rw, rep)
        d_mask.free()


# ---------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors(adac, gpu_ctx):
    a = adac.Layout(gpu_ctx, np.uint32, np.array([10, 20], dtype=np.uint32))
    b = adac.Layout(gpu_ctx, np.uint8, np.array([10, 21], dtype=np.uint32))
    c = adac.Layout(gpu_ctx, np.uint8, np.array([10, 20], dtype=np.uint32))
    d = gpu_ctx.alloc(4096).zero()
    for keys, g, sums in ((b, 4, d), (c, 0, d), (c, 257, d), (c, 4, None)):
        for mask in (d, None):
            with pytest.raises(adac.AdacError):
                a.scan_group_sum_valid(d, keys, d, mask, g, sums, d)
