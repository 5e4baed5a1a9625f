"""adac_scan_sum_product: SUM(a * b) over two packed columns of one table under a selection bitmap (Q6's aggregate).
The expected value is numpy over the ORIGINAL columns: each widened to 64 bits by its own signedness, viewed as uint64,
multiplied and summed with dtype=uint64 (which wraps mod 2^64, as the ABI says).  d_sums is poisoned with 0xFF bytes
before every call and every call is made twice."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

TYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64]
INVALID_ARGUMENT = 1
FULL = 2 ** 64


def widen(v):
    return v.astype(np.int64 if v.dtype.kind == "i" else np.uint64).view(np.uint64)


def expected_sums(a, b, counts, keep=None):
    p = widen(a) * widen(b)
    if keep is not None:
        p = p * keep.astype(np.uint64)
    out, pos = [], 0
    for c in counts:
        out.append(int(p[pos:pos + int(c)].sum(dtype=np.uint64)))
        pos += int(c)
    return out


def offsets_of(counts, val_offs):
    if val_offs is not None:
        return [int(o) for o in val_offs]
    return [int(o) for o in np.concatenate([[0], np.cumsum(counts)[:-1]])]


def encode_column(adac, ctx, vals, counts, val_offs=None, rule=0, pad=False):
    """vals: the rows of all segments back to back -> (layout, packed words); the segments sit at val_offs."""
    counts = np.asarray(counts, dtype=np.uint32)
    lay = adac.Layout(ctx, vals.dtype, counts, val_offs)
    host = np.zeros(max(int(lay.value_span), 1), dtype=vals.dtype)
    pos = 0
    for c, o in zip(counts, offsets_of(counts, val_offs)):
        host[o:o + int(c)] = vals[pos:pos + int(c)]
        pos += int(c)
    d_vals = ctx.upload(host)
    d_words = ctx.alloc(lay.max_arena_words * 8 + 16).zero()
    lay.encode(d_vals, d_words, rule=rule, pad_to_byte=pad)
    ctx.sync()
    return lay, d_words


def place_mask(keep, counts, offs, span):
    """bool per row -> u64 words of a mask over an element space where segment i starts at offs[i] (+ a spare word).
    The elements between the segments are set: they belong to no row and must not matter."""
    full = np.ones(max(span, 1), dtype=bool)
    pos = 0
    for c, o in zip(counts, offs):
        full[int(o):int(o) + int(c)] = keep[pos:pos + int(c)]
        pos += int(c)
    b = np.packbits(full, bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 8 + 8, np.uint8)]).view(np.uint64)


def product_sums(ctx, a, a_words, b, b_words, nseg, d_validity=None):
    """The call, twice, each time into a poisoned result."""
    d_sums = ctx.alloc(max(nseg, 1) * 8 + 8)
    got = []
    for _ in range(2):
        d_sums.upload(np.full(nseg + 1, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
        a.scan_sum_product(a_words, b, b_words, d_sums, d_validity)
        out = d_sums.download(np.uint64, nseg + 1)
        assert int(out[nseg]) == 0xFFFFFFFFFFFFFFFF  # nothing past nseg results
        got.append([int(x) for x in out[:nseg]])
    assert got[0] == got[1]
    d_sums.free()
    return got[0]


def segment_at_width(rng, dtype, n, w):
    """n values of `dtype` that the append rule packs at exactly w bits (n >= 2; w == the type's width: a range that
    does not shrink).  Signed types: the range stays on one side of zero, as the rule's sign-extended order needs."""
    dtype = np.dtype(dtype)
    tb = 8 * dtype.itemsize
    u = np.dtype("u%d" % dtype.itemsize)
    if w >= tb:
        r = rng.integers(0, 2 ** tb - 1, size=n, dtype=np.uint64, endpoint=True)
        if n >= 2:
            r[0], r[1] = (0, 2 ** tb - 1) if dtype.kind == "u" else (2 ** (tb - 1) - 1, 2 ** (tb - 1))
        return r.astype(u).view(dtype)
    span = 2 ** w - 1
    if dtype.kind == "u":
        base = int(rng.integers(0, 2 ** tb - 1 - span, dtype=np.uint64, endpoint=True))
    else:  # bit patterns [0, 2^(tb-1)) are >= 0, [2^(tb-1), 2^tb) are negative
        half = int(rng.integers(0, 2)) * 2 ** (tb - 1)
        base = half + int(rng.integers(0, 2 ** (tb - 1) - 1 - span, dtype=np.uint64, endpoint=True))
    if rng.random() < 0.25:  # large frames of reference: the top of the range
        base = (2 ** tb - 1 - span) if dtype.kind == "u" or rng.random() < 0.5 else (2 ** (tb - 1) - 1 - span)
    r = rng.integers(2 ** (w - 1), span, size=n, dtype=np.uint64, endpoint=True) if n < 2 else \
        rng.integers(0, span, size=n, dtype=np.uint64, endpoint=True)
    if n >= 2:
        r[0], r[n - 1] = 0, span
    return (r + np.uint64(base)).astype(u).view(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# Case 1: every width pair of the two 8-byte types
# ---------------------------------------------------------------------------------------------------------------------
ROWS1 = 333


def width_grid_columns(dtype, seed):
    """64 x 64 segments of 333 rows: segment (i, j) holds a at width i + 1 and b at width j + 1."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([segment_at_width(rng, dtype, ROWS1, s // 64 + 1) for s in range(4096)])
    b = np.concatenate([segment_at_width(rng, dtype, ROWS1, s % 64 + 1) for s in range(4096)])
    return a, b


@pytest.fixture(scope="module", params=[np.uint64, np.int64], ids=["uint64", "int64"])
def width_grid(request):
    dtype = np.dtype(request.param)
    a, b = width_grid_columns(dtype, 640 + (dtype.kind == "i"))
    return dtype, a, b


def test_width_grid_generator_reaches_every_width(oracle, width_grid):
    """Held on the CPU: by the reference's own width rule the generator reaches every (wa, wb) in 1..63 (and 64)."""
    dtype, a, b = width_grid
    wa = [oracle.width_from_succinct(int(s.min()), int(s.max())) for s in a.view(np.uint64).reshape(4096, ROWS1)]
    wb = [oracle.width_from_succinct(int(s.min()), int(s.max())) for s in b.view(np.uint64).reshape(4096, ROWS1)]
    assert wa == [s // 64 + 1 for s in range(4096)]
    assert wb == [s % 64 + 1 for s in range(4096)]
    if dtype.kind == "i":
        assert (a < 0).any() and (b < 0).any() and (a > 0).any()


@gpu
def test_every_width_pair_of_the_8_byte_types(adac, gpu_ctx, width_grid):
    dtype, a, b = width_grid
    counts = np.full(4096, ROWS1, dtype=np.uint32)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    ad, bd = alay.get_descs(), blay.get_descs()
    reached = {(int(x), int(y)) for x, y, fx, fy in zip(ad["width"], bd["width"], ad["flags"], bd["flags"])
               if (fx & adac.SEG_PACKED) and (fy & adac.SEG_PACKED)}
    missing = [(x, y) for x in range(1, 64) for y in range(1, 64) if (x, y) not in reached]
    assert not missing, missing[:8]
    assert not (ad["flags"][63 * 64:] & adac.SEG_PACKED).any()  # a width that does not shrink: unpacked
    exp = (widen(a) * widen(b)).reshape(4096, ROWS1).sum(axis=1, dtype=np.uint64)
    assert len({int(x) for x in exp}) > 4000  # the products wrap all over 2^64
    got = product_sums(gpu_ctx, alay, awords, blay, bwords, 4096)
    bad = [s for s in range(4096) if got[s] != int(exp[s])]
    assert not bad, [(s // 64 + 1, s % 64 + 1) for s in bad[:8]]


# ---------------------------------------------------------------------------------------------------------------------
# Case 2: every type pair
# ---------------------------------------------------------------------------------------------------------------------
COUNTS2 = np.array(([0, 1, 31, 64, 2047, 2048, 2049, 4097, 32767, 65534, 70001] * 4)[:40], dtype=np.uint32)


@pytest.fixture(scope="module")
def typed_columns(adac, gpu_ctx):
    """One 40-segment column per type at random widths, encoded once and shared by the 64 pairs."""
    cols = {}
    rng = np.random.default_rng(2)
    keep = rng.random(int(COUNTS2.sum())) < 0.5
    for t in TYPES:
        t = np.dtype(t)
        vals = np.concatenate([segment_at_width(rng, t, int(c), int(rng.integers(1, 8 * t.itemsize + 1)))
                               for c in COUNTS2])
        cols[t.name] = (vals,) + encode_column(adac, gpu_ctx, vals, COUNTS2)
    d_mask = gpu_ctx.upload(place_mask(keep, COUNTS2, offsets_of(COUNTS2, None), int(COUNTS2.sum())))
    return cols, keep, d_mask


@gpu
@pytest.mark.parametrize("atype", [np.dtype(t).name for t in TYPES])
def test_every_type_pair(adac, gpu_ctx, typed_columns, atype):
    cols, keep, d_mask = typed_columns
    a, alay, awords = cols[atype]
    for btype in (np.dtype(t).name for t in TYPES):
        b, blay, bwords = cols[btype]
        got = product_sums(gpu_ctx, alay, awords, blay, bwords, len(COUNTS2))
        assert got == expected_sums(a, b, COUNTS2), (atype, btype)
        assert got[0] == 0  # the empty segment
        got = product_sums(gpu_ctx, alay, awords, blay, bwords, len(COUNTS2), d_mask)
        assert got == expected_sums(a, b, COUNTS2, keep), (atype, btype, "masked")


# ---------------------------------------------------------------------------------------------------------------------
# Case 3: segment kinds on either side
# ---------------------------------------------------------------------------------------------------------------------
COUNTS3 = np.array([5000, 333, 2049], dtype=np.uint32)


def kind_columns():
    """name -> (values, rule, pad_to_byte, check(descs)); rules: 0 = append, 1 = recompact"""
    rng = np.random.default_rng(3)
    n = int(COUNTS3.sum())
    i32 = np.iinfo(np.int32)
    wrap32 = ((np.uint64(i32.max - 100) + rng.integers(0, 200, size=n).astype(np.uint64)) & np.uint64(0xFFFFFFFF)) \
        .astype(np.uint32).view(np.int32)  # {INT_MAX - 100 .. INT_MIN + 99}: the zero-extended order packs it
    packed, unpacked = (lambda d: all(d["flags"] & 1)), (lambda d: not any(d["flags"] & 1))
    return {
        "int8 across zero": (rng.integers(-128, 128, size=n).astype(np.int8), 0, False, unpacked),
        "int32 full range": (rng.integers(i32.min, i32.max, size=n, endpoint=True).astype(np.int32), 0, False, unpacked),
        "int32 wraps the sign boundary": (wrap32, 1, False, lambda d: all(d["flags"] & 1) and all(d["width"] <= 8)),
        "int16 frame near the top": (rng.integers(32000, 32768, size=n).astype(np.int16), 0, False,
                                     lambda d: all(d["flags"] & 1) and all(d["width"] == 10)),
        "constant": (np.full(n, 7, dtype=np.uint32), 0, False, lambda d: all(d["width"] == 1)),
        "all -1 int64": (np.full(n, -1, dtype=np.int64), 0, False, packed),
        "all -1 int32": (np.full(n, -1, dtype=np.int32), 0, False, packed),
        "padded to bytes": (rng.integers(1000, 1000 + 2 ** 13, size=n).astype(np.uint32), 0, True,
                            lambda d: all(d["width"] == 16)),
        "recompact rule": (rng.integers(300, 20000, size=n).astype(np.uint16), 1, False, packed),
    }


@gpu
def test_segment_kinds_on_either_side(adac, gpu_ctx):
    enc = {}
    for name, (vals, rule, pad, check) in kind_columns().items():
        lay, words = encode_column(adac, gpu_ctx, vals, COUNTS3, rule=rule, pad=pad)
        assert check(lay.get_descs()), (name, lay.get_descs())
        enc[name] = (vals, lay, words)
    assert any(int(m) == 0xFFFFFFFFFFFFFFFF - 1 for m in enc["all -1 int64"][1].get_descs()["min"])  # defect 7's stored min
    for an, (a, alay, awords) in enc.items():
        for bn, (b, blay, bwords) in enc.items():
            got = product_sums(gpu_ctx, alay, awords, blay, bwords, len(COUNTS3))
            assert got == expected_sums(a, b, COUNTS3), (an, bn)


# ---------------------------------------------------------------------------------------------------------------------
# Case 4: the mask, in a's element space
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("atype,btype,abits,bbits", [(np.int32, np.uint16, 21, 9), (np.int64, np.int8, 40, 5),
                                                     (np.uint8, np.uint32, 6, 30)])
def test_mask_in_a_element_space(adac, gpu_ctx, atype, btype, abits, bbits):
    rng = np.random.default_rng(4 + abits)
    counts = np.array([1, 70, 2048, 9000, 0, 333, 4097, 64, 31, 20000] * 3, dtype=np.uint32)
    n = int(counts.sum())
    aoffs = np.cumsum(rng.integers(0, 71, size=len(counts)) + np.concatenate([[0], counts[:-1]])).astype(np.uint64)
    boffs = np.cumsum(rng.integers(0, 71, size=len(counts)) + np.concatenate([[0], counts[:-1]])).astype(np.uint64)
    assert len({int(o) & 63 for o in aoffs}) > 10  # segments start at many bit phases of a mask word
    assert (aoffs != boffs).any()
    a = np.concatenate([segment_at_width(rng, atype, int(c), abits) for c in counts])
    b = np.concatenate([segment_at_width(rng, btype, int(c), bbits) for c in counts])
    alay, awords = encode_column(adac, gpu_ctx, a, counts, aoffs)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts, boffs)
    span = max(int(alay.value_span), int(blay.value_span))
    ends = np.zeros(n, dtype=bool)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)[counts > 0]
    ends[first] = True
    ends[(np.cumsum(counts) - 1)[counts > 0]] = True
    masks = {"ones": np.ones(n, dtype=bool), "zeros": np.zeros(n, dtype=bool), "half": rng.random(n) < 0.5,
             "one percent": rng.random(n) < 0.01, "first and last rows": ends}
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts)) == expected_sums(a, b, counts)
    for name, keep in masks.items():
        d_mask = gpu_ctx.upload(place_mask(keep, counts, aoffs, span))
        got = product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts), d_mask)
        assert got == expected_sums(a, b, counts, keep), name
        if name == "zeros":
            assert not any(got)
        d_mask.free()
    # the same rows kept, but the mask laid out in b's element space: a different answer, so the space used is a's
    keep = masks["half"]
    d_mask = gpu_ctx.upload(place_mask(keep, counts, boffs, span))
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts), d_mask) != expected_sums(a, b, counts, keep)


# ---------------------------------------------------------------------------------------------------------------------
# Case 5: the Q6 chain
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_q6_chain_at_200000_rows(adac, gpu_ctx):
    rng = np.random.default_rng(1994)
    n = 200_000
    cols = {"l_shipdate": rng.integers(8036, 10562, size=n).astype(np.int32),
            "l_discount": rng.integers(0, 11, size=n).astype(np.int32),
            "l_quantity": rng.integers(1, 51, size=n).astype(np.int32),
            "l_extendedprice": rng.integers(90_000, 10_495_000, size=n).astype(np.int32)}
    counts = adac.appender_segment_counts(n, 4)
    enc = {name: encode_column(adac, gpu_ctx, v, counts) for name, v in cols.items()}
    bm = [gpu_ctx.alloc((n + 63) // 64 * 8 + 8) for _ in range(3)]
    d_cnt = gpu_ctx.alloc(len(counts) * 8)
    int_min = int(np.array([np.iinfo(np.int32).min]).view(np.uint32)[0])
    enc["l_shipdate"][0].scan_select_between(enc["l_shipdate"][1], 8766, 9130, bm[0], d_cnt)
    enc["l_discount"][0].scan_select_between(enc["l_discount"][1], 5, 7, bm[1], d_cnt, bm[0])
    enc["l_quantity"][0].scan_select_between(enc["l_quantity"][1], int_min, 23, bm[2], d_cnt, bm[1])
    m = ((cols["l_shipdate"] >= 8766) & (cols["l_shipdate"] <= 9130) & (cols["l_discount"] >= 5) &
         (cols["l_discount"] <= 7) & (cols["l_quantity"] < 24))
    assert int(d_cnt.download(np.uint64, len(counts)).sum()) == int(m.sum()) > 1000
    got = product_sums(gpu_ctx, enc["l_extendedprice"][0], enc["l_extendedprice"][1], enc["l_discount"][0],
                       enc["l_discount"][1], len(counts), bm[2])
    assert sum(got) % FULL == int((cols["l_extendedprice"][m].astype(np.int64) * cols["l_discount"][m]).sum())
    assert got == expected_sums(cols["l_extendedprice"], cols["l_discount"], counts, m)


# ---------------------------------------------------------------------------------------------------------------------
# Case 6: a is b
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype,bits", [(np.uint32, 19), (np.int16, 11)])
def test_a_is_b_gives_the_sum_of_squares(adac, gpu_ctx, dtype, bits):
    rng = np.random.default_rng(6)
    counts = np.array([70001, 333, 0, 4097], dtype=np.uint32)
    x = np.concatenate([segment_at_width(rng, dtype, int(c), bits) for c in counts])
    lay, words = encode_column(adac, gpu_ctx, x, counts)
    got = product_sums(gpu_ctx, lay, words, lay, words, len(counts))
    assert got == expected_sums(x, x, counts)
    sq = x.astype(object) ** 2
    assert got[1] == int(sq[70001:70001 + 333].sum()) % FULL


# ---------------------------------------------------------------------------------------------------------------------
# Case 7: knobs and re-encoded descriptors
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_grouping_knob_and_reencode_leave_the_sums_alone(adac, gpu_ctx):
    rng = np.random.default_rng(7)
    counts = np.array([65534, 70001, 2049, 32767], dtype=np.uint32)
    n = int(counts.sum())
    a = np.concatenate([segment_at_width(rng, np.int32, int(c), 13) for c in counts])
    b = np.concatenate([segment_at_width(rng, np.uint64, int(c), w) for c, w in zip(counts, (5, 40, 64, 31))])
    keep = rng.random(n) < 0.3
    d_mask = gpu_ctx.upload(place_mask(keep, counts, offsets_of(counts, None), n))
    wide, wide_words = encode_column(adac, gpu_ctx, a, counts, pad=True)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    exp, exp_masked = expected_sums(a, b, counts), expected_sums(a, b, counts, keep)
    try:
        for per in (2, 4, 16, 0):
            adac.set_tuning("scan_tiles_per_wg", per)
            assert product_sums(gpu_ctx, wide, wide_words, blay, bwords, len(counts)) == exp, per
            assert product_sums(gpu_ctx, wide, wide_words, blay, bwords, len(counts), d_mask) == exp_masked, per
            assert product_sums(gpu_ctx, blay, bwords, wide, wide_words, len(counts)) == exp, per
    finally:
        adac.set_tuning("scan_tiles_per_wg", 0)
    # the same layout pair (alay, blay) while alay's descriptors change: padded widths first, then the tight ones
    alay = adac.Layout(gpu_ctx, np.int32, counts)
    awords = gpu_ctx.alloc(alay.max_arena_words * 8 + 16).zero()
    wide.reencode(wide_words, alay, awords, pad_to_byte=True)
    assert set(alay.get_descs()["width"].tolist()) == {16}
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts), d_mask) == exp_masked
    wide.reencode(wide_words, alay, awords)
    assert set(alay.get_descs()["width"].tolist()) == {13}
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts), d_mask) == exp_masked
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts)) == exp


# ---------------------------------------------------------------------------------------------------------------------
# Case 8: refusals, all decided on the host before any launch
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_codec_usable(adac, gpu_ctx):
    rng = np.random.default_rng(8)
    counts = np.array([100, 3000], dtype=np.uint32)
    a = np.concatenate([segment_at_width(rng, np.uint32, int(c), 17) for c in counts])
    b = np.concatenate([segment_at_width(rng, np.int8, int(c), 4) for c in counts])
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    d_sums = gpu_ctx.alloc(64)
    other_counts = adac.Layout(gpu_ctx, np.int8, np.array([100, 3001], dtype=np.uint32))
    ctx2 = adac.Context(0)
    try:
        other_ctx = adac.Layout(ctx2, np.int8, counts)
        refused = [lambda: alay.scan_sum_product(awords, other_counts, bwords, d_sums),
                   lambda: alay.scan_sum_product(awords, other_ctx, bwords, d_sums),
                   lambda: alay.scan_sum_product(awords.ptr + 8, blay, bwords, d_sums),
                   lambda: alay.scan_sum_product(awords, blay, bwords.ptr + 8, d_sums),
                   lambda: alay.scan_sum_product(None, blay, bwords, d_sums),
                   lambda: alay.scan_sum_product(awords, blay, bwords, None)]
        for call in refused:
            with pytest.raises(adac.AdacError) as e:
                call()
            assert e.value.status == INVALID_ARGUMENT
        other_ctx.close()
    finally:
        ctx2.close()
    assert product_sums(gpu_ctx, alay, awords, blay, bwords, len(counts)) == expected_sums(a, b, counts)
