"""What the two pair-scan test files share (adac_bp_scan_sum_product, adac_bp_scan_group_sum): columns compressed by
the oracle's restatement of the reference's BITPACKING compress, their decoded rows placed in the element space, the
four masks and the numpy side of both aggregates.  The conventions are tests/test_gpu_bitpacking_scans.py's: expected
values from numpy over the oracle's scan of the same blocks, every output pre-filled with 0xA5 plus a guard word,
every call made twice."""
import numpy as np

from oracle import bitpacking as bp

ALL = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
STRIDE = 262144
GUARD = 0xA5A5A5A5A5A5A5A5
GROUP = 2048


def host_blocks(comp):
    """The segments of a Compressed column as one buffer, block i at i * STRIDE, + the layout's offs and counts."""
    buf = np.zeros(comp.nseg * STRIDE + 64, dtype=np.uint8)
    for i in range(comp.nseg):
        buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE] = comp.block(i)
    offs = np.arange(comp.nseg, dtype=np.uint64) * np.uint64(STRIDE)
    counts = np.array([comp.count(i) for i in range(comp.nseg)], dtype=np.uint32)
    return buf, offs, counts


def pack_bits(mask, nwords):
    """bools over the element space -> nwords + 1 mask words"""
    full = np.zeros(nwords * 64 + 64, dtype=bool)
    full[:len(mask)] = mask
    return np.packbits(full, bitorder="little").view(np.uint64)


def kind_column(dtype, rng, kinds, tail=777):
    """One 2048-row group per entry of `kinds` (test_gpu_bitpacking_scans.mixed_column's five kinds: constant,
    constant delta, sorted small steps -> DELTA_FOR, narrow FOR, wide FOR) and a `tail`-row tail."""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    half = int(info.max) // 2
    parts = []
    for g, kind in enumerate(kinds):
        n = GROUP
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
    if tail:
        parts.append(half // 5 + rng.integers(0, 50, size=tail))
    return np.concatenate(parts).astype(dtype)


def widen(v):
    """The rows as uint64 bit patterns after widening by the type's own signedness."""
    return v.astype(np.int64 if v.dtype.kind == "i" else np.uint64).view(np.uint64)


class Packed:
    """A column as BITPACKING blocks (host side only): the block buffer, the segment table, what the oracle decodes
    from the blocks and every metadata group's (mode, width).  counts: compress these row ranges as one segment each
    instead of letting the codec cut the column into blocks.  validity: the NULL mask the column is compressed under
    (rows that are NULL decode to whatever the codec left there).  phase: segment i starts at element phase + its
    first row."""

    def __init__(self, v, force_mode=bp.MODE_AUTO, counts=None, out_offs=None, validity=None, phase=0):
        v = np.ascontiguousarray(v)
        self.dtype = v.dtype
        nz = validity is not None
        if counts is None:
            comp = bp.Compressed(v, validity, force_mode, null_zero=nz)
            self.buf, self.offs, self.counts = host_blocks(comp)
            comps = [(comp, i) for i in range(comp.nseg)]
        else:
            self.counts = np.asarray(counts, dtype=np.uint32)
            assert int(self.counts.sum()) == len(v)
            self.buf = np.zeros(len(counts) * STRIDE + 64, dtype=np.uint8)
            self.offs = np.arange(len(counts), dtype=np.uint64) * np.uint64(STRIDE)
            comps, row = [], 0
            for i, c in enumerate(self.counts):
                if c:
                    comp = bp.Compressed(v[row:row + int(c)], validity[row:row + int(c)] if nz else None, force_mode,
                                         null_zero=nz)
                    assert comp.nseg == 1
                    self.buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE] = comp.block(0)
                    comps.append((comp, 0))
                else:
                    comps.append((None, 0))
                row += int(c)
        self.segs = [np.zeros(0, self.dtype) if c is None else c.scan(i) for c, i in comps]
        self.nseg = len(self.counts)
        if out_offs is None and phase:
            out_offs = phase + np.concatenate([[0], np.cumsum(self.counts[:-1], dtype=np.uint64)]).astype(np.uint64)
        self.out_offs = (np.concatenate([[0], np.cumsum(self.counts[:-1], dtype=np.uint64)]).astype(np.uint64)
                         if out_offs is None else np.asarray(out_offs, dtype=np.uint64))
        self.explicit_offs = out_offs is not None
        self.span = max([int(o) + len(s) for o, s in zip(self.out_offs, self.segs)], default=0)
        self.nwords = (self.span + 63) // 64
        # the element space: widened rows where a segment covers the element
        self.wide = np.zeros(self.span, dtype=np.uint64)
        self.raw = np.zeros(self.span, dtype=self.dtype)
        self.cover = np.zeros(self.span, dtype=bool)
        self.modes = []       # (mode, width) of every metadata group, in the order of the layout's group table
        self.group_start = []  # element offset of every group
        for (c, i), o, s in zip(comps, self.out_offs, self.segs):
            o = int(o)
            self.wide[o:o + len(s)] = widen(s)
            self.raw[o:o + len(s)] = s
            self.cover[o:o + len(s)] = True
            for g in range((len(s) + GROUP - 1) // GROUP):
                mode, _, w = c.group_info(i, g)
                self.modes.append((mode, w))
                self.group_start.append(o + g * GROUP)


class Dev:
    """A Packed column on the device: the uploaded blocks and the layout."""

    def __init__(self, adac, ctx, packed):
        self.ctx, self.p = ctx, packed
        self.d_blocks = ctx.upload(packed.buf)
        self.lay = adac.BitpackingLayout(ctx, packed.dtype, packed.offs, packed.counts,
                                         packed.out_offs if packed.explicit_offs else None)
        assert self.lay.value_span == packed.span
        assert self.lay.ngroups == len(packed.modes)


def fresh(ctx, nwords):
    """An output buffer holding 0xA5 in every byte (+ a guard word)."""
    return ctx.alloc(nwords * 8 + 8).upload(np.full(nwords * 8 + 8, 0xA5, dtype=np.uint8))


def untouched(d_buf, nwords):
    return bool(np.all(d_buf.download(np.uint64, nwords + 1) == np.uint64(GUARD)))


def four_masks(span, rng):
    """all-zero, all-one, 50 % random, and whole 64-row steps clear with the others full."""
    steps = rng.random((span + 63) // 64) < 0.5
    return {"zero": np.zeros(span, dtype=bool), "one": np.ones(span, dtype=bool), "random": rng.random(span) < 0.5,
            "steps": np.repeat(steps, 64)[:span]}


def full_mask(a, mask):
    m = np.ones(a.span, dtype=bool) if mask is None else np.asarray(mask[:a.span], dtype=bool)
    return m & a.cover


def want_sum_product(a, b, mask):
    """Per segment of a: sum of widen(a) * widen(b) mod 2^64 over the selected rows."""
    keep = full_mask(a, mask)
    n = min(a.span, b.span)
    assert np.array_equal(a.cover[:n], b.cover[:n]) and not a.cover[n:].any() and not b.cover[n:].any()
    prod = np.zeros(a.span, dtype=np.uint64)
    prod[:n] = a.wide[:n] * b.wide[:n]          # uint64 arithmetic wraps
    out = []
    for o, s in zip(a.out_offs, a.segs):
        o = int(o)
        out.append(int(prod[o:o + len(s)][keep[o:o + len(s)]].sum(dtype=np.uint64)))
    return out


def check_sum_product(da, db, mask=None, d_valid=None, mask_words=None):
    """mask: bools over the element space (may be longer than the span: bits past it must change nothing)."""
    a, b, ctx = da.p, db.p, da.ctx
    want = want_sum_product(a, b, mask)
    if mask is not None and d_valid is None:
        d_valid = ctx.upload(pack_bits(mask, a.nwords) if mask_words is None else mask_words)
    for _ in range(2):
        d_sums = fresh(ctx, a.nseg)
        da.lay.scan_sum_product(da.d_blocks, db.lay, db.d_blocks, d_sums, d_valid)
        got = d_sums.download(np.uint64, a.nseg + 1)
        assert [int(x) for x in got[:-1]] == want
        assert int(got[-1]) == GUARD
    return want


def want_group_sum(v, k, ngroups, mask):
    keep = full_mask(v, mask)
    n = min(v.span, k.span)
    assert np.array_equal(v.cover[:n], k.cover[:n])
    keys = k.raw[:n].view("u%d" % k.dtype.itemsize).astype(np.uint64)   # unsigned, of the key type's own width
    bins = np.minimum(keys, np.uint64(ngroups)).astype(np.int64)[keep[:n]]
    vals = v.wide[:n][keep[:n]]
    sums = np.zeros(ngroups + 1, dtype=np.uint64)
    np.add.at(sums, bins, vals)
    counts = np.bincount(bins, minlength=ngroups + 1).astype(np.uint64)
    return [int(x) for x in sums], [int(x) for x in counts]


def check_group_sum(dv, dk, ngroups, mask=None, d_valid=None, with_counts=True):
    v, k, ctx = dv.p, dk.p, dv.ctx
    want_s, want_c = want_group_sum(v, k, ngroups, mask)
    if mask is not None and d_valid is None:
        d_valid = ctx.upload(pack_bits(mask, v.nwords))
    for _ in range(2):
        d_sums, d_counts = fresh(ctx, ngroups + 1), fresh(ctx, ngroups + 1)
        dv.lay.scan_group_sum(dv.d_blocks, dk.lay, dk.d_blocks, ngroups, d_sums, d_counts if with_counts else None,
                              d_valid)
        got = d_sums.download(np.uint64, ngroups + 2)
        assert [int(x) for x in got[:-1]] == want_s
        assert int(got[-1]) == GUARD
        if with_counts:
            got = d_counts.download(np.uint64, ngroups + 2)
            assert [int(x) for x in got[:-1]] == want_c
            assert int(got[-1]) == GUARD
        else:
            assert untouched(d_counts, ngroups + 1)
    return want_s, want_c
