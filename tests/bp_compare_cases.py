"""What the tests of adac_bp_scan_select_compare / adac_bp_scan_count_compare share: the numpy side of a comparison
between two columns of DuckDB BITPACKING blocks and the check of one call.  The columns, the device side and the
conventions are tests/bp_pair_cases.py's: expected values from numpy over the oracle's scan of the same blocks, every
output pre-filled with 0xA5 plus a guard word, every call made twice, the bitmap compared word for word over all of
its words."""
import numpy as np

from bp_pair_cases import GROUP, GUARD, STRIDE, fresh, full_mask, pack_bits
from oracle import bitpacking as bp

LT, EQ, GT = 1, 2, 4                # ADAC_CMP_*
ALL_CMPS = [1, 2, 3, 4, 5, 6]       # LT, EQ, LE, GT, NE, GE
LINEAR, FOR, DELTA = "linear", "for", "delta"


def relation(a, b):
    """Per element of a's space: which of LT / EQ / GT the rows of two Packed columns answer to, the raw values compared
    as mathematical integers (Python ints, whatever the two types are); 0 where no segment covers the element."""
    n = min(a.span, b.span)
    assert np.array_equal(a.cover[:n], b.cover[:n]) and not a.cover[n:].any() and not b.cover[n:].any()
    x, y = a.raw[:n].astype(object), b.raw[:n].astype(object)
    rel = np.zeros(a.span, dtype=np.uint8)
    rel[:n] = np.where(np.asarray(x < y, dtype=bool), LT, np.where(np.asarray(x == y, dtype=bool), EQ, GT))
    rel[~a.cover] = 0
    return rel


def want_compare(a, rel, cmp, mask):
    """(bools over a's element space, rows selected per segment of a) for one comparison under one mask"""
    bits = full_mask(a, mask) & ((rel & np.uint8(cmp)) != 0)
    counts = [int(bits[int(o):int(o) + len(s)].sum()) for o, s in zip(a.out_offs, a.segs)]
    return bits, counts


def check_select_compare(da, db, cmp, mask=None, d_valid=None, mask_words=None, rel=None, count_form=True):
    """Both forms of the call against numpy.  mask: bools over the element space (may be longer than the span: bits
    past it must change nothing); d_valid: the same mask already on the device; rel: relation(da.p, db.p) when the
    caller has it.  Returns (the selected elements as bools, the counts, the device bitmap of the last call)."""
    a, ctx = da.p, da.ctx
    rel = relation(a, db.p) if rel is None else rel
    bits, counts = want_compare(a, rel, cmp, mask)
    words = pack_bits(bits, a.nwords)[:a.nwords]
    if mask is not None and d_valid is None:
        d_valid = ctx.upload(pack_bits(mask, a.nwords) if mask_words is None else mask_words)
    d_bitmap = None
    for _ in range(2):
        d_bitmap, d_counts = fresh(ctx, a.nwords), fresh(ctx, a.nseg)
        da.lay.scan_select_compare(da.d_blocks, db.lay, db.d_blocks, cmp, d_bitmap, d_counts, d_valid)
        got = d_bitmap.download(np.uint64, a.nwords + 1)
        bad = np.flatnonzero(got[:-1] != words)
        assert len(bad) == 0, "cmp %d: %d bitmap words differ, the first at %d: %#x != %#x" % (
            cmp, len(bad), bad[0], int(got[bad[0]]), int(words[bad[0]]))
        assert int(got[-1]) == GUARD
        got = d_counts.download(np.uint64, a.nseg + 1)
        assert [int(x) for x in got[:-1]] == counts, cmp
        assert int(got[-1]) == GUARD
    for _ in range(2 if count_form else 0):
        d_counts = fresh(ctx, a.nseg)
        da.lay.scan_count_compare(da.d_blocks, db.lay, db.d_blocks, cmp, d_counts, d_valid)
        got = d_counts.download(np.uint64, a.nseg + 1)
        assert [int(x) for x in got[:-1]] == counts, cmp
        assert int(got[-1]) == GUARD
    return bits, counts, d_bitmap


def cursor_kinds(p):
    """How the pair kernels' cursor reads every metadata group of a Packed column: linear (CONSTANT, CONSTANT_DELTA,
    width 0), FOR or DELTA_FOR at a width of at least 1."""
    return [LINEAR if m not in (bp.MODE_FOR, bp.MODE_DELTA_FOR) or w == 0 else FOR if m == bp.MODE_FOR else DELTA
            for m, w in p.modes]


def for_payloads(p):
    """(byte offset in p.buf, bytes) of the packed fields of every FOR group of a Packed column at a width of at least
    1, read from the block images as bp_fuzz_columns.segment_groups reads the headers."""
    ts = p.dtype.itemsize
    out = []
    for i, rows in enumerate(int(c) for c in p.counts):
        blk = p.buf[i * STRIDE:i * STRIDE + bp.BLOCK_SIZE]
        if rows == 0:
            continue
        first = int(blk[:8].view(np.uint64)[0])
        for g in range((rows + GROUP - 1) // GROUP):
            enc = int(blk[first - 4 * (g + 1):first - 4 * g].view(np.uint32)[0])
            mode, off = enc >> 24, enc & 0xffffff
            width = int(blk[off + ts])          # (bitpacking_width_t) of the header's second word, little endian
            if mode == bp.MODE_FOR and width:
                n = min(GROUP, rows - g * GROUP)
                out.append((i * STRIDE + off + 2 * ts, (n + 31) // 32 * 32 * width // 8))
    return out
