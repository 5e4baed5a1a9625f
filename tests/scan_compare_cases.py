"""Columns, expected values and the call wrapper shared by the tests of adac_scan_select_compare /
adac_scan_count_compare (test_scan_compare_forms.py on the CPU, test_gpu_scan_select_compare*.py on the GPU).

Expected values are numpy over the ORIGINAL columns.  The comparison is made exact for mixed signedness by hand: both
sides are widened to 64 bits by their own signedness, and a negative value of the signed side is below every value of the
unsigned one (compare_masks; held against Python integers in test_scan_compare_forms.py)."""
import numpy as np

from test_gpu_sum_product import TYPES, encode_column, offsets_of, place_mask, segment_at_width  # noqa: F401

POISON = 0xFFFFFFFFFFFFFFFF
LT, EQ, GT = 1, 2, 4
CMPS = (1, 2, 3, 4, 5, 6)
NO_MIN = 0xFFFFFFFFFFFFFFFF


def compare_masks(a, b):
    """(a < b, a == b, a > b) per row as mathematical integers, whatever the two integer dtypes are"""
    sa, sb = a.dtype.kind == "i", b.dtype.kind == "i"
    if sa == sb:
        x, y = (a.astype(np.int64), b.astype(np.int64)) if sa else (a.astype(np.uint64), b.astype(np.uint64))
        return x < y, x == y, x > y
    if sb:  # a unsigned, b signed: the mirror image
        gt, eq, lt = compare_masks(b, a)
        return lt, eq, gt
    neg = a < 0
    x, y = a.astype(np.int64).view(np.uint64), b.astype(np.uint64)
    return neg | (x < y), ~neg & (x == y), ~neg & (x > y)


def hits_of(masks, cmp, keep=None):
    lt, eq, gt = masks
    h = np.zeros(len(lt), dtype=bool)
    if cmp & LT:
        h |= lt
    if cmp & EQ:
        h |= eq
    if cmp & GT:
        h |= gt
    return h if keep is None else h & keep


def place_bits(hit, counts, offs, span):
    """bool per row -> the ceil(span / 64) bitmap words; elements between the segments are zero"""
    full = np.zeros(((max(span, 0) + 63) // 64) * 64, dtype=bool)
    pos = 0
    for c, o in zip(counts, offs):
        full[int(o):int(o) + int(c)] = hit[pos:pos + int(c)]
        pos += int(c)
    return np.packbits(full, bitorder="little").view(np.uint64) if len(full) else np.zeros(0, np.uint64)


def seg_counts(hit, counts):
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    cs = np.concatenate([[0], np.cumsum(hit, dtype=np.int64)])
    return [int(cs[e] - cs[e - int(c)]) for e, c in zip(ends, counts)]


def run_compare(ctx, alay, awords, blay, bwords, cmp, d_validity=None):
    """Select twice and count twice, each into poisoned outputs with a spare word -> (bitmap words, counts)"""
    nseg, nwords = len(alay.counts), (int(alay.value_span) + 63) // 64
    d_bm, d_cnt = ctx.alloc(nwords * 8 + 8), ctx.alloc(nseg * 8 + 8)
    got = []
    for _ in range(2):
        d_bm.upload(np.full(nwords + 1, POISON, dtype=np.uint64))
        d_cnt.upload(np.full(nseg + 1, POISON, dtype=np.uint64))
        alay.scan_select_compare(awords, blay, bwords, cmp, d_bm, d_cnt, d_validity)
        bm, cn = d_bm.download(np.uint64, nwords + 1), d_cnt.download(np.uint64, nseg + 1)
        assert int(bm[nwords]) == POISON and int(cn[nseg]) == POISON  # nothing past the results
        got.append((bm[:nwords].copy(), [int(x) for x in cn[:nseg]]))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]
    for _ in range(2):
        d_cnt.upload(np.full(nseg + 1, POISON, dtype=np.uint64))
        alay.scan_count_compare(awords, blay, bwords, cmp, d_cnt, d_validity)
        cn = d_cnt.download(np.uint64, nseg + 1)
        assert int(cn[nseg]) == POISON
        assert [int(x) for x in cn[:nseg]] == got[0][1], "the count form disagrees with the select's counts"
    d_bm.free()
    d_cnt.free()
    return got[0]


def check_compare(ctx, a, alay, awords, b, blay, bwords, counts, cmps=CMPS, keep=None, d_mask=None, val_offs=None,
                  what=""):
    """every cmp of cmps against numpy: bitmap, counts, the count form; LT + EQ + GT add up to the wanted rows"""
    masks = compare_masks(a, b)
    offs = offsets_of(counts, val_offs)
    span = int(alay.value_span)
    single = {}
    for cmp in cmps:
        bm, cn = run_compare(ctx, alay, awords, blay, bwords, cmp, d_mask)
        hit = hits_of(masks, cmp, keep)
        exp_cn = seg_counts(hit, counts)
        bad = [s for s in range(len(counts)) if cn[s] != exp_cn[s]]
        assert not bad, (what, cmp, [(s, cn[s], exp_cn[s]) for s in bad[:6]])
        exp_bm = place_bits(hit, counts, offs, span)
        wrong = np.nonzero(bm != exp_bm)[0]
        assert len(wrong) == 0, (what, cmp, [(int(w), hex(int(bm[w])), hex(int(exp_bm[w]))) for w in wrong[:4]])
        single[cmp] = cn
    if all(c in single for c in (LT, EQ, GT)):
        wanted = seg_counts(np.ones(len(a), dtype=bool) if keep is None else keep, counts)
        assert [x + y + z for x, y, z in zip(single[LT], single[EQ], single[GT])] == wanted, what


# ---------------------------------------------------------------------------------------------------------------------
# two columns of one type whose value intervals overlap: the same base on both sides
# ---------------------------------------------------------------------------------------------------------------------
def pick_base(rng, dtype, w):
    """bit pattern of a frame that keeps [base, base + 2^w - 1] inside the type and on one side of zero (w < type bits)"""
    tb, span = 8 * dtype.itemsize, 2 ** w - 1
    if dtype.kind == "u":
        base = int(rng.integers(0, 2 ** tb - 1 - span, dtype=np.uint64, endpoint=True))
    else:
        half = int(rng.integers(0, 2)) * 2 ** (tb - 1)
        base = half + int(rng.integers(0, 2 ** (tb - 1) - 1 - span, dtype=np.uint64, endpoint=True))
    if rng.random() < 0.25:
        base = (2 ** tb - 1 - span) if dtype.kind == "u" or rng.random() < 0.5 else (2 ** (tb - 1) - 1 - span)
    return base


def full_range(rng, dtype, n):
    tb = 8 * dtype.itemsize
    r = rng.integers(0, 2 ** tb - 1, size=n, dtype=np.uint64, endpoint=True)
    r[0], r[n - 1] = (0, 2 ** tb - 1) if dtype.kind == "u" else (2 ** (tb - 1) - 1, 2 ** (tb - 1))  # the type's max, min
    return r


def pair_at_widths(rng, dtype, n, wa, wb):
    """(a, b): n >= 8 rows of `dtype` that the append rule packs at exactly wa and wb bits (the type's width: a range
    that does not shrink), both from ONE base so that the intervals overlap.  Rows 0, 1, 2 are an EQ, an LT and a GT
    pair, row n - 1 pins both ranges' upper ends; of the others about 1/8 have b = a and 1/8 b = a +- 1 where the other
    side's range holds the value.  (A side at the type's width is random over the whole type, its ends pinned in rows
    0 and n - 1, and takes the planted rows.)"""
    dtype = np.dtype(dtype)
    tb, u = 8 * dtype.itemsize, np.dtype("u%d" % dtype.itemsize)
    tmask = np.uint64(2 ** tb - 1)
    mid = np.arange(3, n - 1)
    pick = rng.random(len(mid))
    same, near = mid[pick < 0.125], mid[(pick >= 0.125) & (pick < 0.25)]
    step = rng.integers(0, 2, size=len(near)).astype(np.uint64)
    if wa >= tb or wb >= tb:
        wide = full_range(rng, dtype, n)
        w = min(wa, wb)
        if w >= tb:
            other = full_range(rng, dtype, n)
        else:
            base, span = pick_base(rng, dtype, w), 2 ** w - 1
            f = rng.integers(0, span, size=n, dtype=np.uint64, endpoint=True)
            f[0], f[n - 1] = 0, span
            other = (f + np.uint64(base)) & tmask
        # the full-range side can hold any value of the other: plant there (LT and GT come with the random rows)
        wide[same] = other[same]
        wide[near] = (other[near] + np.uint64(2) * step - np.uint64(1)) & tmask
        a, b = (wide, other) if wa >= tb else (other, wide)
        return a.astype(u).view(dtype), b.astype(u).view(dtype)
    base = pick_base(rng, dtype, max(wa, wb))
    sa, sb = 2 ** wa - 1, 2 ** wb - 1
    fa = rng.integers(0, sa, size=n, dtype=np.uint64, endpoint=True)
    fb = rng.integers(0, sb, size=n, dtype=np.uint64, endpoint=True)
    fb[same] = np.minimum(fa[same], np.uint64(sb))
    up = np.minimum(fa[near] + np.uint64(1), np.uint64(sb))
    down = np.minimum(np.where(fa[near] > 0, fa[near] - np.uint64(1), np.uint64(0)), np.uint64(sb))
    fb[near] = np.where(step == 1, up, down)
    fa[0], fb[0] = 0, 0      # EQ
    fa[1], fb[1] = 0, 1      # LT
    fa[2], fb[2] = 1, 0      # GT
    fa[n - 1], fb[n - 1] = sa, sb
    a, b = (fa + np.uint64(base)) & tmask, (fb + np.uint64(base)) & tmask
    return a.astype(u).view(dtype), b.astype(u).view(dtype)


ROWS_GRID = 333
GRID32 = [(wa, wb) for wa in range(1, 33) for wb in range(1, 33)]
W64 = (1, 3, 4, 5, 31, 32, 33, 63, 64)
GRID64 = [(wa, wb) for wa in W64 for wb in W64]


def width_grid_columns(dtype):
    dtype = np.dtype(dtype)
    grid = GRID32 if dtype.itemsize == 4 else GRID64
    rng = np.random.default_rng(1200 + 8 * dtype.itemsize + (dtype.kind == "i"))
    pairs = [pair_at_widths(rng, dtype, ROWS_GRID, wa, wb) for wa, wb in grid]
    return grid, np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


# ---------------------------------------------------------------------------------------------------------------------
# one column per type for the 8 x 8 type pairs: three segments of 257 rows
# ---------------------------------------------------------------------------------------------------------------------
COUNTS_TYPES = np.array([257, 257, 257], dtype=np.uint32)


def specials(dtype):
    info = np.iinfo(dtype)
    s = [info.min, info.max, 0, 1]
    if dtype.kind == "i":
        s.append(-1)
    if dtype.itemsize == 8:
        s.append(2 ** 63 - 1)
        if dtype.kind == "u":
            s += [2 ** 63, 2 ** 63 + 1]
    return s


def typed_column(dtype, side=0):
    """segment 0: the whole range with the type's special values; 1: small values (equal across the types);
    2: the top of the type, for uint64 both sides of 2^63.  side: 0 for the a column, 1 for the b column (another draw)"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1300 + 8 * dtype.itemsize + (dtype.kind == "i") + 100 * side)
    n, info, u = 257, np.iinfo(dtype), np.dtype("u%d" % dtype.itemsize)
    s0 = rng.integers(0, 2 ** (8 * dtype.itemsize) - 1, size=n, dtype=np.uint64, endpoint=True).astype(u).view(dtype)
    sp = specials(dtype)
    s0[:len(sp)] = np.array([v & (2 ** (8 * dtype.itemsize) - 1) for v in sp], dtype=np.uint64).astype(u).view(dtype)
    s0[8:16] = np.array([[5, 1, 3, 0, 2, 2, 7, 7], [1, 5, 3, 2, 0, 2, 6, 8]][side], dtype=dtype)  # GT, LT, EQ in any type pair
    s1 = rng.integers(0, 8, size=n).astype(dtype)
    if dtype == np.uint64:
        s2 = (np.uint64(2 ** 63 - 8) + rng.integers(0, 16, size=n).astype(np.uint64)).astype(dtype)
    else:
        s2 = (np.uint64(info.max) - rng.integers(0, 16, size=n).astype(np.uint64)).astype(u).view(dtype)
    return np.concatenate([s0, s1, s2])


# ---------------------------------------------------------------------------------------------------------------------
# the descriptor the encoder writes for a segment, by the reference's width rule (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def oracle_descs(orc, adac, vals, counts, rule=0, padded=False):
    d = np.zeros(len(counts), dtype=adac.SEGMENT_DESC_DTYPE)
    tb, pos = 8 * vals.dtype.itemsize, 0
    for i, c in enumerate(counts):
        v = vals[pos:pos + int(c)]
        pos += int(c)
        d["count"][i] = int(c)
        if int(c) == 0:
            d["width"][i], d["min"][i] = tb, NO_MIN
            continue
        mn, mx = orc.analyze_flat(v, rule)
        w = (orc.width_from_succinct if rule == 0 else orc.width_from_uncompressed)(mn, mx, padded)
        packed = tb > w
        d["width"][i], d["flags"][i], d["min"][i] = (w if packed else tb), int(packed), (mn if packed else NO_MIN)
    return d


def math_range(v):
    return int(v.min()), int(v.max())


# ---------------------------------------------------------------------------------------------------------------------
# segment pairs for the header form (int32, 5000 rows each) with the form compare_plan gives each
# ---------------------------------------------------------------------------------------------------------------------
def header_columns():
    rng = np.random.default_rng(1400)
    n = 5000

    def between(lo, hi):
        v = rng.integers(lo, hi, size=n, endpoint=True).astype(np.int32)
        v[0], v[n - 1] = lo, hi
        return v

    def const(c):
        return np.full(n, c, dtype=np.int32)

    pairs = [
        (between(1000, 2023), between(3000, 4023), "header"),      # a wholly below b
        (between(3000, 4023), between(10, 1033), "header"),        # a wholly above b
        (between(-4023, -3000), between(-2000, -977), "header"),   # both below zero
        (between(1000, 2023), between(2023, 3046), "fast"),        # touching: max(a) == min(b)
        (between(2023, 3046), between(1000, 2023), "fast"),        # touching: min(a) == max(b)
        (const(7), const(7), "generic"),                           # constants pack at one bit: [7, 8] twice
        (const(7), const(500), "header"),
        (const(500), const(7), "header"),
        (const(-3), const(40000), "header"),
        (between(-4023, -3000), between(-100, 923), "generic"),    # b crosses zero: raw signed slots, no frame
    ]
    counts = np.full(len(pairs), n, dtype=np.uint32)
    return (np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]), counts,
            [p[2] for p in pairs])
