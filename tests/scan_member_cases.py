"""The reference, the columns and the call wrappers shared by the tests of adac_scan_select_member /
adac_scan_count_member / adac_scan_build_member (test_scan_member_forms.py on the CPU, test_gpu_scan_member*.py on the
GPU).

Expected values are numpy over the ORIGINAL columns.  A domain is (base, bits): base a bit pattern of the column type,
the values base ... base + bits - 1 in the type's own order.  The index of a value is taken in the order-preserving
map B(v) = bits(v) ^ sign bit, t = B(v) - B(base) mod 2^64, in the domain iff t < bits (member_index; held against
Python integers in test_scan_member_forms.py)."""
import numpy as np

from test_gpu_sum_product import TYPES, encode_column, offsets_of, place_mask, segment_at_width  # noqa: F401
from scan_compare_cases import place_bits, seg_counts  # noqa: F401

POISON = 0xFFFFFFFFFFFFFFFF
SLICE_BITS = 65536


def kind(dtype):
    dtype = np.dtype(dtype)
    return (dtype.itemsize, dtype.kind == "i")


def sign_bit(dtype):
    dtype = np.dtype(dtype)
    return (1 << (8 * dtype.itemsize - 1)) if dtype.kind == "i" else 0


def pattern(dtype, value):
    """the zero-extended bit pattern of a value of the type"""
    return int(value) & ((1 << (8 * np.dtype(dtype).itemsize)) - 1)


def biased(vals):
    """B(v) = bits(v) ^ sign bit as uint64: the type's own order as an unsigned one"""
    u = np.dtype("u%d" % vals.dtype.itemsize)
    return vals.view(u).astype(np.uint64) ^ np.uint64(sign_bit(vals.dtype))


def member_index(vals, base, bits):
    """(t, inside): the set index of every row (mod 2^64) and whether the row's value lies in the domain"""
    t = biased(vals) - np.uint64(base ^ sign_bit(vals.dtype))
    return t, (t <= np.uint64(bits - 1))


def set_words_for(bits):
    return (bits + 63) // 64


def member_mask(vals, base, bits, set_words, keep=None):
    """rows selected by the probe: wanted, in the domain, set bit 1 (bits >= `bits` of the last word are no members)"""
    t, inside = member_index(vals, base, bits)
    ti = np.where(inside, t, np.uint64(0))
    bit = (set_words[(ti >> np.uint64(6)).astype(np.int64)] >> (ti & np.uint64(63))) & np.uint64(1)
    hit = inside & (bit != 0)
    return hit if keep is None else hit & keep


def built_set(vals, base, bits, keep=None):
    """(the set the build writes, the wanted rows in the domain)"""
    t, inside = member_index(vals, base, bits)
    if keep is not None:
        inside = inside & keep
    words = np.zeros(set_words_for(bits), dtype=np.uint64)
    idx = t[inside]
    np.bitwise_or.at(words, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    return words, inside


def random_set(rng, bits, density=0.5, tail_ones=True):
    """a set of `bits` bits; every bit of the last word at a position >= bits is SET (they must never select a row)"""
    n = set_words_for(bits)
    if density == 0.5:
        words = rng.integers(0, POISON, size=n, dtype=np.uint64, endpoint=True)
    else:
        words = np.packbits(rng.random(n * 64) < density, bitorder="little").view(np.uint64).copy()
    if bits % 64:
        low = np.uint64((1 << (bits % 64)) - 1)
        words[-1] = (words[-1] | ~low) if tail_ones else (words[-1] & low)
    return words


def set_bit(words, i, on):
    if on:
        words[i >> 6] |= np.uint64(1 << (i & 63))
    else:
        words[i >> 6] &= np.uint64(~(1 << (i & 63)) & POISON)


# ---------------------------------------------------------------------------------------------------------------------
# the calls, twice each, into poisoned outputs with a spare word
# ---------------------------------------------------------------------------------------------------------------------
def run_member(ctx, lay, words, d_set, base, bits, d_validity=None):
    """Select twice and count twice -> (bitmap words, counts)"""
    nseg, nwords = len(lay.counts), (int(lay.value_span) + 63) // 64
    d_bm, d_cnt = ctx.alloc(nwords * 8 + 8), ctx.alloc(nseg * 8 + 8)
    got = []
    for _ in range(2):
        d_bm.upload(np.full(nwords + 1, POISON, dtype=np.uint64))
        d_cnt.upload(np.full(nseg + 1, POISON, dtype=np.uint64))
        lay.scan_select_member(words, d_set, base, bits, d_bm, d_cnt, d_validity)
        bm, cn = d_bm.download(np.uint64, nwords + 1), d_cnt.download(np.uint64, nseg + 1)
        assert int(bm[nwords]) == POISON and int(cn[nseg]) == POISON  # nothing past the results
        got.append((bm[:nwords].copy(), [int(x) for x in cn[:nseg]]))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    for _ in range(2):
        d_cnt.upload(np.full(nseg + 1, POISON, dtype=np.uint64))
        lay.scan_count_member(words, d_set, base, bits, d_cnt, d_validity)
        cn = d_cnt.download(np.uint64, nseg + 1)
        assert int(cn[nseg]) == POISON
        assert [int(x) for x in cn[:nseg]] == got[0][1], "the count form disagrees with the select's counts"
    d_bm.free()
    d_cnt.free()
    return got[0]


def run_build(ctx, lay, words, base, bits, d_validity=None):
    """Build twice into a poisoned set -> (set words, counts)"""
    nseg, nset = len(lay.counts), set_words_for(bits)
    d_set, d_cnt = ctx.alloc(nset * 8 + 8), ctx.alloc(nseg * 8 + 8)
    got = []
    for _ in range(2):
        d_set.upload(np.full(nset + 1, POISON, dtype=np.uint64))
        d_cnt.upload(np.full(nseg + 1, POISON, dtype=np.uint64))
        lay.scan_build_member(words, base, bits, d_set, d_cnt, d_validity)
        st, cn = d_set.download(np.uint64, nset + 1), d_cnt.download(np.uint64, nseg + 1)
        assert int(st[nset]) == POISON and int(cn[nseg]) == POISON
        got.append((st[:nset].copy(), [int(x) for x in cn[:nseg]]))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    d_set.free()
    d_cnt.free()
    return got[0]


def check_member(ctx, vals, lay, words, counts, base, bits, set_words, keep=None, d_mask=None, val_offs=None, what=""):
    """the probe against numpy: bitmap, counts, the count form"""
    d_set = ctx.upload(set_words)
    bm, cn = run_member(ctx, lay, words, d_set, base, bits, d_mask)
    d_set.free()
    hit = member_mask(vals, base, bits, set_words, keep)
    exp_cn = seg_counts(hit, counts)
    bad = [s for s in range(len(counts)) if cn[s] != exp_cn[s]]
    assert not bad, (what, [(s, cn[s], exp_cn[s]) for s in bad[:6]])
    exp_bm = place_bits(hit, counts, offsets_of(counts, val_offs), int(lay.value_span))
    wrong = np.nonzero(bm != exp_bm)[0]
    assert len(wrong) == 0, (what, [(int(w), hex(int(bm[w])), hex(int(exp_bm[w]))) for w in wrong[:4]])
    return hit


def check_build(ctx, vals, lay, words, counts, base, bits, keep=None, d_mask=None, what=""):
    """the build against numpy: the set (its tail bits zero) and the rows in the domain per segment"""
    st, cn = run_build(ctx, lay, words, base, bits, d_mask)
    exp_set, inside = built_set(vals, base, bits, keep)
    exp_cn = seg_counts(inside, counts)
    assert cn == exp_cn, (what, [(s, cn[s], exp_cn[s]) for s in range(len(counts)) if cn[s] != exp_cn[s]][:6])
    wrong = np.nonzero(st != exp_set)[0]
    assert len(wrong) == 0, (what, [(int(w), hex(int(st[w])), hex(int(exp_set[w]))) for w in wrong[:4]])
    return exp_set


# ---------------------------------------------------------------------------------------------------------------------
# the width grid: one segment per width 1 ... 8 * sizeof(T), each with a domain of its own INSIDE its interval, and rows
# of all four classes planted: below the domain, inside on a set bit, inside on a clear bit, above the domain
# ---------------------------------------------------------------------------------------------------------------------
ROWS_GRID = 257
GRID_TYPES = (np.int32, np.uint32, np.int64, np.uint64)


def unbias(b, dtype):
    """uint64 biased numbers -> values of the type"""
    dtype = np.dtype(dtype)
    u = np.dtype("u%d" % dtype.itemsize)
    return (np.asarray(b, dtype=np.uint64) ^ np.uint64(sign_bit(dtype))).astype(u).view(dtype)


def grid_segment(rng, dtype, w, cap_bits):
    """(values, base, bits, set words) for one segment at width w.  segment_at_width pins the interval's ends in rows
    0, 1 and n - 1; rows 2 ... 129 are planted: 32 below the domain, 32 on set bits, 32 on clear bits, 32 above.
    At w = 1 a segment holds two values: the domain is both, one on a set and one on a clear bit."""
    dtype = np.dtype(dtype)
    v = segment_at_width(rng, dtype, ROWS_GRID, w)
    b = biased(v)
    bmin, bmax = int(b.min()), int(b.max())
    if w == 1:
        dlo, bits = bmin, 2
        words = np.array([POISON & ~2], dtype=np.uint64)   # bit 0 set, bit 1 clear, the tail set
        return v, dlo ^ sign_bit(dtype), bits, words
    extent = bmax - bmin + 1
    bits = max(2, min(extent // 2, cap_bits))
    dlo = bmin + max(1, (extent - bits) // 2)
    dhi = dlo + bits - 1
    assert bmin < dlo and dhi < bmax
    words = random_set(rng, bits)
    k = 32
    below = rng.integers(bmin, dlo - 1, size=k, dtype=np.uint64, endpoint=True)
    above = rng.integers(dhi + 1, bmax, size=k, dtype=np.uint64, endpoint=True)
    t_on = rng.integers(0, bits // 2 - 1, size=k, dtype=np.uint64, endpoint=True) * np.uint64(2)       # even indices
    t_off = t_on + np.uint64(1)                                                                         # odd, <= bits - 1
    for t in t_on:
        set_bit(words, int(t), True)
    for t in t_off:
        set_bit(words, int(t), False)
    planted = np.concatenate([below, np.uint64(dlo) + t_on, np.uint64(dlo) + t_off, above])
    v[2:2 + 4 * k] = unbias(planted, dtype)
    return v, dlo ^ sign_bit(dtype), bits, words


def width_grid(dtype):
    """[(base, bits, set words)] per segment and the column of all segments back to back"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(2100 + 8 * dtype.itemsize + (dtype.kind == "i"))
    segs = []
    for w in range(1, 8 * dtype.itemsize + 1):
        cap = (SLICE_BITS // 2, SLICE_BITS + 1, 1 << 20)[w % 3]   # windows on both sides of the slice limit
        segs.append(grid_segment(rng, dtype, w, cap))
    return np.concatenate([s[0] for s in segs]), [s[1:] for s in segs]


def classes_of(vals, base, bits, set_words):
    """which of the four classes occur among the rows"""
    t, inside = member_index(vals, base, bits)
    hit = member_mask(vals, base, bits, set_words)
    b, dlo = biased(vals), np.uint64(base ^ sign_bit(vals.dtype))
    return {"below": bool((~inside & (b < dlo)).any()), "set": bool(hit.any()), "clear": bool((inside & ~hit).any()),
            "above": bool((~inside & (b > dlo)).any())}


# ---------------------------------------------------------------------------------------------------------------------
# one column per type: three segments of 257 rows (the whole range with the ends of the type, small values, the top)
# and the domains that start at the type's minimum, end at its maximum and straddle zero
# ---------------------------------------------------------------------------------------------------------------------
def typed_domains(dtype):
    """[(name, base pattern, bits)]"""
    dtype = np.dtype(dtype)
    info, tb = np.iinfo(dtype), 8 * dtype.itemsize
    span = min(1 << 24, 1 << tb)
    out = [("from the minimum", pattern(dtype, info.min), min(span, 300)),
           ("to the maximum", pattern(dtype, info.max - (min(span, 300) - 1)), min(span, 300)),
           ("one bit at the maximum", pattern(dtype, info.max), 1),
           ("one bit at the minimum", pattern(dtype, info.min), 1),
           ("small values", pattern(dtype, 2), 5)]
    if dtype.kind == "i":
        out.append(("straddles zero", pattern(dtype, -100), 201))
        out.append(("one bit at minus one", pattern(dtype, -1), 1))
    if tb <= 16:
        out.append(("the whole type", pattern(dtype, info.min), 1 << tb))
    else:
        out.append(("2^24 bits to the maximum", pattern(dtype, info.max - ((1 << 24) - 1)), 1 << 24))
        out.append(("2^24 bits from the minimum", pattern(dtype, info.min), 1 << 24))
    return out
