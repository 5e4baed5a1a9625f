"""Fused scans on DuckDB BITPACKING blocks (adac_bp_scan_sum / _count_between / _select_between / _min_max): blocks
written by the oracle's restatement of the reference's compress, scanned on the device without a decode, compared
with numpy over the oracle's scan of the same blocks.  Before every call every output buffer is filled with 0xA5 and
every call is made twice: nothing may depend on what the outputs held."""
import numpy as np
import pytest

from oracle import bitpacking as bp

pytestmark = pytest.mark.gpu
ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
STRIDE = 262144
M64 = (1 << 64) - 1


def bits_of(x, dtype):
    dtype = np.dtype(dtype)
    return int(np.array([x], dtype=dtype).view("u%d" % dtype.itemsize)[0])


def mixed_column(dtype, rng, groups=9):
    """test_gpu_bitpacking.mixed_column's shape: constant, constant delta, delta_for, for groups and a 777-row tail."""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    half = int(info.max) // 2
    parts = []
    for g in range(groups):
        n = 2048
        kind = g % 5
        if kind == 0:
            parts.append(np.full(n, half // 3 + g, dtype=np.int64))
        elif kind == 1:
            parts.append(7 + (3 * np.arange(n, dtype=np.int64)) % max(half - 7, 1))
        elif kind == 2:
            steps = rng.integers(0, 3, size=n)
            parts.append(half // 2 + np.cumsum(steps) % (half // 4 + 1))
            parts[-1].sort()
        elif kind == 3:
            span = min(8 * dtype.itemsize - 2, 13)
            parts.append(half // 3 + rng.integers(0, 1 << span, size=n))
        else:
            lo = int(info.min) // 2 if dtype.kind == "i" else 0
            parts.append(rng.integers(lo, half, size=n, dtype=np.int64))
    parts.append(half // 5 + rng.integers(0, 50, size=777))
    return np.concatenate(parts).astype(dtype)


def host_blocks(comp):
    buf = np.zeros(comp.nseg * STRIDE + 64, dtype=np.uint8)
    for i in range(comp.nseg):
        buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE] = comp.block(i)
    offs = np.arange(comp.nseg, dtype=np.uint64) * np.uint64(STRIDE)
    counts = np.array([comp.count(i) for i in range(comp.nseg)], dtype=np.uint32)
    return buf, offs, counts


def pack_bits(mask, nwords):
    full = np.zeros(nwords * 64 + 64, dtype=bool)
    full[:len(mask)] = mask
    return np.packbits(full, bitorder="little").view(np.uint64)


class Column:
    """A layout over uploaded blocks + what the oracle decodes from them, segment by segment."""

    def __init__(self, adac, ctx, dtype, buf, offs, counts, segs, out_offs=None):
        self.adac, self.ctx, self.dtype = adac, ctx, np.dtype(dtype)
        self.d_blocks = ctx.upload(buf)
        self.segs = segs
        self.out_offs = (np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.uint64)]).astype(np.uint64)
                         if out_offs is None else np.asarray(out_offs, dtype=np.uint64))
        self.lay = adac.BitpackingLayout(ctx, dtype, offs, counts, None if out_offs is None else self.out_offs)
        self.nseg = len(counts)
        self.span = max([int(o) + len(s) for o, s in zip(self.out_offs, segs)], default=0)
        assert self.lay.value_span == self.span
        self.nwords = (self.span + 63) // 64

    @classmethod
    def from_values(cls, adac, ctx, v, force_mode=bp.MODE_AUTO, out_offs=None, validity=None, phase=0):
        """validity: the NULL mask the column is compressed under.  phase: segment i starts at element phase + its
        first row."""
        comp = bp.Compressed(v, validity, force_mode, null_zero=validity is not None)
        buf, offs, counts = host_blocks(comp)
        if out_offs is None and phase:
            out_offs = phase + np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.uint64)]).astype(np.uint64)
        col = cls(adac, ctx, v.dtype, buf, offs, counts, [comp.scan(i) for i in range(comp.nseg)], out_offs)
        col.comp = comp
        return col

    def fresh(self, nwords):  # an output buffer holding 0xA5 in every byte (+ a guard word)
        return self.ctx.alloc(nwords * 8 + 8).upload(np.full(nwords * 8 + 8, 0xA5, dtype=np.uint8))

    def keep(self, i, mask):
        o, n = int(self.out_offs[i]), len(self.segs[i])
        return np.ones(n, dtype=bool) if mask is None else mask[o:o + n]

    def check_sum_min_max(self, mask=None, d_valid=None):
        info = np.iinfo(self.dtype)
        wide = np.int64 if self.dtype.kind == "i" else np.uint64
        if mask is not None and d_valid is None:
            d_valid = self.ctx.upload(pack_bits(mask, self.nwords))
        want_sum, want_mm = [], []
        for i, s in enumerate(self.segs):
            live = s[self.keep(i, mask)]
            want_sum.append(int(live.astype(wide).view(np.uint64).sum(dtype=np.uint64)))
            want_mm += ([bits_of(live.min(), self.dtype), bits_of(live.max(), self.dtype)] if len(live)
                        else [bits_of(info.max, self.dtype), bits_of(info.min, self.dtype)])
        for _ in range(2):
            d_sum, d_mm = self.fresh(self.nseg), self.fresh(2 * self.nseg)
            self.lay.scan_sum(self.d_blocks, d_sum, d_valid)
            self.lay.scan_min_max(self.d_blocks, d_mm, d_valid)
            got = d_sum.download(np.uint64, self.nseg + 1)
            assert [int(x) for x in got[:-1]] == want_sum
            assert int(got[-1]) == 0xA5A5A5A5A5A5A5A5
            got = d_mm.download(np.uint64, 2 * self.nseg + 1)
            assert [int(x) for x in got[:-1]] == want_mm
            assert int(got[-1]) == 0xA5A5A5A5A5A5A5A5
        return want_sum, want_mm

    def check_range(self, lo, hi, mask=None, d_valid=None):
        """lo, hi: values of the column type.  Returns the expected selection over the span."""
        if mask is not None and d_valid is None:
            d_valid = self.ctx.upload(pack_bits(mask, self.nwords))
        sel = np.zeros(self.span, dtype=bool)
        want = []
        lo_t, hi_t = self.dtype.type(lo), self.dtype.type(hi)
        for i, s in enumerate(self.segs):
            hit = (s >= lo_t) & (s <= hi_t) & self.keep(i, mask)
            o = int(self.out_offs[i])
            sel[o:o + len(s)] = hit
            want.append(int(hit.sum()))
        want_words = pack_bits(sel, self.nwords)[:self.nwords]
        blo, bhi = bits_of(lo, self.dtype), bits_of(hi, self.dtype)
        for _ in range(2):
            d_cnt, d_cnt2, d_bm = self.fresh(self.nseg), self.fresh(self.nseg), self.fresh(self.nwords)
            self.lay.scan_count_between(self.d_blocks, blo, bhi, d_cnt, d_valid)
            self.lay.scan_select_between(self.d_blocks, blo, bhi, d_bm, d_cnt2, d_valid)
            for d in (d_cnt, d_cnt2):
                got = d.download(np.uint64, self.nseg + 1)
                assert [int(x) for x in got[:-1]] == want, (lo, hi)
                assert int(got[-1]) == 0xA5A5A5A5A5A5A5A5
            got = d_bm.download(np.uint64, self.nwords + 1)
            bad = np.flatnonzero(got[:-1] != want_words)
            assert len(bad) == 0, (lo, hi, bad[:8], [hex(int(x)) for x in got[bad[:4]]])
            assert int(got[-1]) == 0xA5A5A5A5A5A5A5A5
        return sel


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
def test_all_types_through_every_mode(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(300 + dtype.itemsize + (dtype.kind == "i"))
    v = mixed_column(dtype, rng)
    col = Column.from_values(adac, gpu_ctx, v)
    modes = col.comp.groups_by_mode()
    assert modes["constant"] >= 1 and modes["for"] >= 1, modes
    if dtype.itemsize > 1:
        assert modes["constant_delta"] >= 1 and modes["delta_for"] >= 1, modes
    info = np.iinfo(dtype)
    col.check_sum_min_max()
    present = int(v[5000])
    seen = set(v.tolist())
    absent = next(x for x in range(int(info.max), int(info.min), -1) if x not in seen)
    ranges = [(info.min, info.max), (present, present), (absent, absent), (info.min, int(np.median(v))),
              (int(info.max) // 2, int(info.max) // 2 - 1)]
    if dtype.kind == "i":
        ranges.append((-(int(info.max) // 4), int(info.max) // 4))
    for lo, hi in ranges:
        sel = col.check_range(lo, hi)
        if (lo, hi) == (info.min, info.max):
            assert sel.all()
        if (lo, hi) == (present, present):
            assert sel.any()
        if (lo, hi) == (absent, absent) or lo > hi:
            assert not sel.any()
    mask = rng.random(col.span) < 0.5
    col.check_sum_min_max(mask)
    col.check_range(info.min, int(np.median(v)), mask)


# 2 -----------------------------------------------------------------------------------------------------------------
def width_column(dtype, mode, rng):
    """One 2048-row group per width 0 .. bits - 2 (test_gpu_bitpacking.test_forced_modes_and_widths' generator)."""
    bits = 8 * dtype.itemsize
    cols = []
    for w in range(0, bits - 1):
        span = rng.integers(0, 1 << w, size=2048, dtype=np.uint64) if w else np.zeros(2048, dtype=np.uint64)
        if w:
            span[3], span[9] = 0, (1 << w) - 1
        base = 1000
        if mode == bp.MODE_DELTA_FOR:
            step = np.minimum(span, np.uint64((1 << max(bits - 13, 1)) - 1))
            c = base + np.cumsum(step.astype(object))
            if int(c[-1]) >= (1 << (bits - 1)) - 1:
                continue
            cols.append(np.array(c, dtype=np.uint64))
        else:
            if (1 << w) + base >= (1 << (bits - 1)):
                continue
            cols.append(span + np.uint64(base))
    return cols


@pytest.mark.parametrize("dtype", [np.uint16, np.uint32, np.uint64, np.int32])
@pytest.mark.parametrize("mode", [bp.MODE_FOR, bp.MODE_DELTA_FOR])
def test_every_width(adac, gpu_ctx, dtype, mode):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(9)
    cols = width_column(dtype, mode, rng)
    v = np.concatenate(cols).astype(dtype)
    col = Column.from_values(adac, gpu_ctx, v, force_mode=mode)
    widths = {col.comp.group_info(0, g)[2] for g in range(min(col.comp.count(0) // 2048, 40))}
    assert len(widths) >= (4 if dtype.itemsize == 2 else 12), sorted(widths)
    col.check_sum_min_max()
    # one range per group, cutting that group's own interval in the middle: the selection of the whole column under
    # it is checked, the group itself straddles it
    for g in range(0, len(cols), max(1, len(cols) // 6)):
        c = cols[g]
        mid = (int(c.min()) + int(c.max())) // 2
        col.check_range(int(c.min()) + (1 if g else 0), mid)
    mids = sorted((int(c.min()) + int(c.max())) // 2 for c in cols)
    col.check_range(mids[len(mids) // 3], mids[-1])


# 3 -----------------------------------------------------------------------------------------------------------------
def test_for_interval_shortcuts(adac, gpu_ctx):
    rng = np.random.default_rng(31)
    # groups with intervals [base, base + 1024): below, inside, straddling and above the range
    bases = [1000, 5000, 9000, 13000, 20000, 30000]
    v = np.concatenate([b + rng.integers(0, 1024, size=2048) for b in bases]).astype(np.int32)
    for b in range(len(bases)):
        v[b * 2048], v[b * 2048 + 1] = bases[b], bases[b] + 1023
    col = Column.from_values(adac, gpu_ctx, v, force_mode=bp.MODE_FOR)
    assert col.comp.groups_by_mode()["for"] == len(bases)
    assert all(col.comp.group_info(0, g)[2] == 10 for g in range(len(bases)))
    mask = rng.random(col.span) < 0.5
    for m in (None, mask):
        col.check_range(5000, 13500, m)       # misses 0, 4, 5; covers 1, 2; straddles 3
        col.check_range(4999, 6023, m)        # exactly one group's interval
        col.check_range(5001, 6023, m)        # one short of it at the bottom: per row
        col.check_range(40000, 50000, m)      # misses every group
        col.check_sum_min_max(m)


@pytest.mark.parametrize("dtype", [np.uint8, np.int8, np.uint64, np.int64])
def test_for_interval_that_wraps_the_type(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(5)
    v = (int(info.max) - rng.integers(0, 6, size=2048).astype(object))
    v[0], v[1] = int(info.max) - 5, int(info.max)
    v = np.array(v, dtype=dtype)
    col = Column.from_values(adac, gpu_ctx, v)
    assert col.comp.groups_by_mode() == {"constant": 0, "constant_delta": 0, "delta_for": 0, "for": 1}
    assert col.comp.group_info(0, 0)[2] == 3  # frame + 7 wraps T
    sel = col.check_range(int(info.max) - 2, int(info.max))
    assert sel.any() and not sel.all()
    sel = col.check_range(int(info.min), int(info.min) + 1)  # where the wrapped interval would falsely reach
    assert not sel.any()
    col.check_range(int(info.max) - 5, int(info.max))
    col.check_sum_min_max()


def test_constant_column_many_atomics_on_one_cell(adac, gpu_ctx):
    n = 3_000_000
    v = np.full(n, -123457, dtype=np.int32)
    col = Column.from_values(adac, gpu_ctx, v)
    assert col.nseg == 1 and col.lay.ngroups == 1465
    assert col.comp.groups_by_mode()["constant"] == 1465
    mask = np.random.default_rng(2).random(n) < 0.4
    d_valid = gpu_ctx.upload(pack_bits(mask, col.nwords))
    col.check_sum_min_max(mask, d_valid)
    col.check_range(-123457, -123457, mask, d_valid)
    col.check_range(-123456, 5, mask, d_valid)
    col.check_sum_min_max()
    # the same column with a few CUs' worth of waves: every wave walks a run of groups
    adac.set_tuning("num_cus", 2)
    try:
        col.check_sum_min_max(mask, d_valid)
        col.check_range(-123457, -123457, mask, d_valid)
    finally:
        adac.set_tuning("num_cus", 0)


def test_constant_delta_middle_stretch(adac, gpu_ctx):
    v = (100 + 7 * np.arange(3 * 2048 + 300, dtype=np.int64)).astype(np.int64)
    col = Column.from_values(adac, gpu_ctx, v)
    assert col.comp.groups_by_mode()["constant_delta"] == 4
    sel = col.check_range(100 + 7 * 1000, 100 + 7 * 5000 + 3)
    assert int(sel.sum()) == 4001
    col.check_sum_min_max()
    col.check_sum_min_max(np.random.default_rng(3).random(col.span) < 0.5)


# 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [1, 63, 64, 65, 777])
def test_placement_at_every_bit_phase(adac, gpu_ctx, tail):
    rng = np.random.default_rng(40 + tail)
    counts = np.array([2048 + 18, 2 * 2048 + tail, 2048 + tail], dtype=np.uint32)
    segs = []
    buf = np.zeros(3 * STRIDE + 64, dtype=np.uint8)
    for i, c in enumerate(counts):
        comp = bp.Compressed((rng.integers(0, 1 << 11, size=int(c)) - 700).astype(np.int16))
        assert comp.nseg == 1
        segs.append(comp.scan(0))
        buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE] = comp.block(0)
    offs = np.arange(3, dtype=np.uint64) * np.uint64(STRIDE)
    # A: groups start at bit 3, its last row is bit 20 of a word; B starts at bit 21 of that word; five empty words;
    # C starts at bit 63
    a0 = 2 * 64 + 3
    b0 = a0 + int(counts[0])
    assert b0 % 64 == 21
    c0 = ((b0 + int(counts[1]) + 63) // 64 + 5) * 64 + 63
    col = Column(adac, gpu_ctx, np.int16, buf, offs, counts, segs, [a0, b0, c0])
    mask = rng.random(col.span) < 0.5   # random bits in the gaps too: they must not leak into bitmap or counts
    for m in (None, mask):
        sel = col.check_range(-200, 600, m)
        assert sel.any() and not sel[:a0].any() and not sel[b0 + int(counts[1]):c0].any()
        col.check_range(-32768, 32767, m)
        col.check_sum_min_max(m)
    # the same blocks with group starts at bits 0 and 37
    c0 = ((int(counts[0]) + 63) // 64 + 3) * 64 + 37
    col = Column(adac, gpu_ctx, np.int16, buf, offs, counts, segs, [0, c0 + int(counts[2]) + 64 * 20 - tail, c0])
    assert int(col.out_offs[1]) % 64 == 37 and int(col.out_offs[2]) % 64 == 37
    mask = rng.random(col.span) < 0.5
    for m in (None, mask):
        col.check_range(-200, 600, m)
        col.check_sum_min_max(m)


# 5 -----------------------------------------------------------------------------------------------------------------
def test_multi_segment_results_are_per_segment(adac, gpu_ctx):
    rng = np.random.default_rng(50)
    v = rng.integers(0, 256, size=600_000).astype(np.uint8)
    col = Column.from_values(adac, gpu_ctx, v)
    assert [len(s) for s in col.segs] == [260096, 260096, 79808]
    sums, _ = col.check_sum_min_max()
    assert len(set(sums)) == 3
    mask = rng.random(col.span) < 0.3
    col.check_sum_min_max(mask)
    col.check_range(17, 99, mask)
    col.check_range(17, 99)
    adac.set_tuning("num_cus", 1)   # 32 waves: runs of groups that cross segment boundaries inside one wave
    try:
        col.check_sum_min_max(mask)
        col.check_range(17, 99, mask)
    finally:
        adac.set_tuning("num_cus", 0)
    w = (rng.integers(0, 1 << 32, size=200_000, dtype=np.uint64) + np.uint64(1 << 40)).astype(np.uint64)
    w[0], w[1] = 1 << 40, (1 << 40) + (1 << 32) - 1
    colw = Column.from_values(adac, gpu_ctx, w)
    assert colw.comp.group_info(0, 0)[2] == 32 and colw.nseg >= 2
    colw.check_sum_min_max()
    colw.check_range((1 << 40) + (1 << 30), (1 << 40) + (3 << 30))


# 6 -----------------------------------------------------------------------------------------------------------------
def test_bitmap_chains_into_other_scans(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(60)
    n = 100_000
    x = rng.integers(-500, 500, size=n).astype(np.int16)
    y = (10 ** 11 + rng.integers(0, 1 << 20, size=n)).astype(np.int64)
    counts = np.array([30_000, 50_000, 20_000], dtype=np.uint32)
    starts = np.array([0, 30_000, 80_000])

    def column(v):   # the same three row ranges for both columns: equal out_offs, one element space
        buf = np.zeros(3 * STRIDE + 64, dtype=np.uint8)
        segs = []
        for i in range(3):
            comp = bp.Compressed(v[starts[i]:starts[i] + counts[i]])
            assert comp.nseg == 1
            buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE] = comp.block(0)
            segs.append(comp.scan(0))
        return Column(adac, ctx, v.dtype, buf, np.arange(3, dtype=np.uint64) * np.uint64(STRIDE), counts, segs)

    cx, cy = column(x), column(y)
    d_bm, d_cnt = cx.fresh(cx.nwords), cx.fresh(3)
    cx.lay.scan_select_between(cx.d_blocks, bits_of(-50, np.int16), bits_of(120, np.int16), d_bm, d_cnt)
    sel = (x >= -50) & (x <= 120)
    # expected values from numpy's selection, the device runs under X's bitmap
    want_sums, want_mm = cy.check_sum_min_max(sel, d_bm)
    assert sum(want_sums) & M64 == int(y[sel].sum()) & M64
    # the same bitmap under a succinct scan over the decoded Y in the same element space
    d_y = ctx.alloc(n * 8 + 64)
    cy.lay.unpack(cy.d_blocks, d_y)
    sl = adac.Layout(ctx, np.int64, counts)
    d_words = ctx.alloc(sl.max_arena_words * 8 + 64).zero()
    sl.encode(d_y, d_words)
    d_sum = cx.fresh(3)
    sl.scan_sum(d_words, d_sum, d_bm)
    assert [int(v) for v in d_sum.download(np.uint64, 3)] == want_sums


# 7 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint32, np.int16, np.uint64])
def test_values_are_what_the_decode_defines(adac, gpu_ctx, dtype):
    """A frame of reference overwritten in the uploaded image so that field + frame wraps T: whatever adac_bp_unpack
    makes of the patched bytes is what the scans aggregate."""
    ctx = gpu_ctx
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(70)
    v = (1000 + rng.integers(0, 1 << 9, size=3 * 2048 + 100)).astype(dtype)
    comp = bp.Compressed(v, force_mode=bp.MODE_FOR)
    buf, offs, counts = host_blocks(comp)
    mode, off, w = comp.group_info(0, 1)
    assert mode == bp.MODE_FOR and w == 9
    first = int(buf[:8].view(np.uint64)[0])
    enc = int(buf[first - 8:first - 4].view(np.uint32)[0])     # group 1's metadata entry
    assert enc >> 24 == bp.MODE_FOR and enc & 0xffffff == off
    frame = np.array([int(info.max) - 100], dtype=dtype)        # field + frame passes T's maximum for most rows
    buf[off:off + dtype.itemsize] = frame.view(np.uint8)
    lay = adac.BitpackingLayout(ctx, dtype, offs, counts)
    d_blocks = ctx.upload(buf)
    d_out = ctx.alloc(len(v) * dtype.itemsize + 64)
    lay.unpack(d_blocks, d_out)
    dec = d_out.download(dtype, len(v))
    assert int(dec[2048:4096].min()) < 1000 and not np.array_equal(dec, v)   # the group wrapped
    col = Column(adac, ctx, dtype, buf, offs, counts, [dec])
    col.check_sum_min_max()
    col.check_range(int(info.max) - 50, int(info.max))
    col.check_range(int(info.min), int(info.min) + 200)
    col.check_range(int(info.min), int(info.max))
    col.check_sum_min_max(rng.random(col.span) < 0.5)


# 8 -----------------------------------------------------------------------------------------------------------------
def test_degenerate_layouts_and_arguments(adac, gpu_ctx):
    ctx = gpu_ctx
    empty = adac.BitpackingLayout(ctx, np.int32, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    assert empty.value_span == 0
    d_any = ctx.alloc(64).upload(np.full(64, 0xA5, dtype=np.uint8))
    d_blocks = ctx.alloc(64).zero()
    empty.scan_sum(d_blocks, d_any)
    empty.scan_count_between(d_blocks, 0, 5, d_any)
    empty.scan_select_between(d_blocks, 0, 5, d_any, d_any)
    empty.scan_min_max(d_blocks, d_any)
    empty.scan_sum(None, None)
    assert np.all(d_any.download(np.uint8, 64) == 0xA5)
    # a zero-row segment between two others
    rng = np.random.default_rng(80)
    v = rng.integers(-1000, 1000, size=5000).astype(np.int32)
    a, b = bp.Compressed(v[:3000]), bp.Compressed(v[3000:])
    buf = np.zeros(3 * STRIDE + 64, dtype=np.uint8)
    buf[:bp.BLOCK_SIZE] = a.block(0)
    buf[2 * STRIDE:2 * STRIDE + bp.BLOCK_SIZE] = b.block(0)
    counts = np.array([3000, 0, 2000], dtype=np.uint32)
    col = Column(adac, ctx, np.int32, buf, np.arange(3, dtype=np.uint64) * np.uint64(STRIDE), counts,
                 [a.scan(0), np.zeros(0, np.int32), b.scan(0)])
    sums, mm = col.check_sum_min_max()
    assert sums[1] == 0 and mm[2:4] == [0x7fffffff, 0x80000000]
    col.check_range(-10, 500)
    col.check_range(5, 4)            # lo > hi selects nothing
    # NULL outputs or blocks with rows present, a bitmap that aliases the mask
    d_cnt, d_bm = col.fresh(3), col.fresh(col.nwords)
    for call in (lambda: col.lay.scan_sum(col.d_blocks, None),
                 lambda: col.lay.scan_min_max(col.d_blocks, None),
                 lambda: col.lay.scan_count_between(col.d_blocks, 0, 5, None),
                 lambda: col.lay.scan_select_between(col.d_blocks, 0, 5, None, d_cnt),
                 lambda: col.lay.scan_select_between(col.d_blocks, 0, 5, d_bm, None),
                 lambda: col.lay.scan_select_between(col.d_blocks, 0, 5, d_bm, d_cnt, d_bm),
                 lambda: col.lay.scan_sum(None, d_cnt)):
        with pytest.raises(adac.AdacError) as err:
            call()
        assert err.value.status == 1
