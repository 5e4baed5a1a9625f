"""adac_scan_group_sum_product_mapped: SUM(a * b), SUM(a), COUNT(*) GROUP BY a code looked up through a dense key, on the
packed bytes of three columns.  Expected values are numpy over the ORIGINAL columns (product_mapped_cases.expected); the
comparison is exact.  Every call is made twice into poisoned outputs with one spare word after each, which must stay
poison, and the two results must be equal."""
import numpy as np
import pytest

import dense_cases as dc
import mapped_cases as mc
import product_mapped_cases as pc
import scan_member_cases as sm
from mapped_cases import ALL_FORMS, MAPPED_SLICE, padded
from product_mapped_cases import check_product, expected, product_forms, run_product
from scan_member_cases import POISON
from scan_compare_cases import typed_column, COUNTS_TYPES
from test_gpu_group_dense import Knob, domain_around, segments_of
from test_gpu_group_mapped import ngroups_column, sparse_keys
from test_gpu_scan_select_compare import COUNTS4, gapped_offsets, half_mask
from test_gpu_sum_product import COUNTS3, encode_column, kind_columns, offsets_of

gpu = pytest.mark.gpu
INVALID_ARGUMENT = 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. every key width, each segment with a domain of its own inside its interval; two value columns whose widths cycle
#    independently over 1 ... 16; unmasked and under half_mask; every output combination
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", sm.GRID_TYPES, ids=lambda t: np.dtype(t).name)
def test_key_width_grid(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    keys, a, b, doms = pc.key_width_grid(dtype)
    nseg = 8 * dtype.itemsize
    counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    assert [int(w) for w in klay.get_descs()["width"]] == list(range(1, nseg + 1))
    wa, wb = [int(w) for w in alay.get_descs()["width"]], [int(w) for w in blay.get_descs()["width"]]
    assert len(set(wa)) == 16 and len(set(wb)) == 16 and len(set(zip(wa, wb))) >= 16 and wa != wb
    rng = np.random.default_rng(81)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    seen = set()
    for s, (base, span) in enumerate(doms):
        f = product_forms(klay, base, span, alay, blay)
        assert f[s] not in (None, "header")
        assert f[s].endswith("-slice") == (span <= MAPPED_SLICE), (s + 1, f[s], span)
        seen |= set(f)
        ngroups = mc.NGROUPS[s % len(mc.NGROUPS)]
        codes = mc.draw_map(rng, span, ngroups)
        _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base,
                                        span, ngroups, what=(s + 1,))
        mine = inside[s * sm.ROWS_GRID:(s + 1) * sm.ROWS_GRID]
        assert mine.any() and (s == 0 or not mine.all()), s + 1   # rows inside and outside the domain
        check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups,
                      keep, d_mask, (s + 1, "masked"))
    # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 indices: no staged reader without a slice)
    assert seen >= ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. every width of the 8-byte types on one side against widths 1 + (7 w) % 32 on the other, then the roles swapped; the
#    key at w = 13; products that wrap, negative factors
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("swap", (False, True), ids=("a sweeps", "b sweeps"))
@pytest.mark.parametrize("vtype", [np.uint64, np.int64], ids=lambda t: np.dtype(t).name)
def test_value_widths(adac, gpu_ctx, vtype, swap):
    vtype = np.dtype(vtype)
    keys, sweep, cyc, cyc_w = pc.value_width_columns(vtype)
    a, b = (cyc, sweep) if swap else (sweep, cyc)
    counts = np.full(pc.VW_SEGS, pc.VW_ROWS, dtype=np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    assert all(int(w) == 13 for w in klay.get_descs()["width"])
    widths = ([int(w) for w in alay.get_descs()["width"]], [int(w) for w in blay.get_descs()["width"]])
    assert widths[swap] == list(range(1, 65)) and widths[not swap] == cyc_w
    rng = np.random.default_rng(82)
    ngroups = 3
    for base, span, acc in ((1000 + 200, MAPPED_SLICE, "slice"), (1100, 5000, "direct")):
        f = product_forms(klay, base, span, alay, blay)
        assert f == ["walk-" + acc] * 32 + ["staged-" + acc] * 32, f   # walk while both are <= 32, staged otherwise
        codes = mc.draw_map(rng, span, ngroups)
        sab, sa, c, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes,
                                           base, span, ngroups, what=(acc,), every_output=False)
        assert inside.sum() > 200
    t, _ = sm.member_index(keys, base, span)
    exact_ab, exact_a = [0] * (ngroups + 1), [0] * (ngroups + 1)
    for i in np.nonzero(inside)[0]:
        g = min(int(codes[int(t[i])]), ngroups)
        exact_ab[g] += int(a[i]) * int(b[i])
        exact_a[g] += int(a[i])
    if vtype.kind == "u":
        assert any(x >= 2 ** 64 for x in exact_ab), "no product sum wrapped"
    else:
        ai, bi = a[inside], b[inside]
        assert ((ai < 0) & (bi > 0)).any() or ((ai > 0) & (bi < 0)).any(), "no negative x positive"
        assert ((ai < 0) & (bi < 0)).any(), "no negative x negative"
    assert [int(x) for x in sab] == [x % 2 ** 64 for x in exact_ab]
    assert [int(x) for x in sa] == [x % 2 ** 64 for x in exact_a]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the lanes bound: the key at w = 4 (the most rows per chunk), a and b at 32 / 5, 5 / 32, 32 / 32; 24 577 rows are two
#    scan groups with uneven quarters; then three segments, the last one's key at w = 40 (staged)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wa,wb", pc.LANES_WIDTHS)
def test_lanes_bound(adac, gpu_ctx, wa, wb):
    rng = np.random.default_rng(83)
    for counts, wide in (((24577,), False), ((24577, 4099, 1000), True)):
        keys, a, b, counts = pc.lanes_columns(wa, wb, counts, wide)
        klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
        alay, awords = encode_column(adac, gpu_ctx, a, counts)
        blay, bwords = encode_column(adac, gpu_ctx, b, counts)
        assert [int(w) for w in klay.get_descs()["width"]] == [4] * (len(counts) - wide) + [40] * wide
        assert all(int(w) == wa for w in alay.get_descs()["width"]) and all(int(w) == wb for w in blay.get_descs()["width"])
        keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
        base, span, ngroups = 702, 12, 5
        f = product_forms(klay, base, span, alay, blay)
        assert f == ["walk-slice"] * (len(counts) - wide) + ["staged-slice"] * wide, f
        codes = mc.draw_map(rng, span, ngroups)
        _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base,
                                        span, ngroups, what=(wa, wb, len(counts)), every_output=not wide)
        assert inside.sum() > 10000 and not inside.all()
        check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups,
                      keep, d_mask, (wa, wb, len(counts), "masked"), every_output=False)


# ---------------------------------------------------------------------------------------------------------------------
# 4. ngroups and the maps around it; one bin for every row; the overflow entry for every row; no overflow at 256
# ---------------------------------------------------------------------------------------------------------------------
def product_columns():
    """test_gpu_group_mapped.ngroups_column (walk, walk, staged; `a` negative against a frame) and a second factor"""
    keys, a, counts = ngroups_column()
    b = np.random.default_rng(84).integers(0, 11, size=len(keys)).astype(np.int8)   # one side of zero: packed, walkable
    return keys, a, b, counts


@gpu
@pytest.mark.parametrize("ngroups", mc.NGROUPS)
def test_ngroups(adac, gpu_ctx, ngroups):
    keys, a, b, counts = product_columns()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    rng = np.random.default_rng(85 + ngroups)
    for base, span in ((1000 + 5, 8000), (2000, MAPPED_SLICE - 7)):
        f = product_forms(klay, base, span, alay, blay)
        assert f == (["walk-direct", "walk-direct", "staged-direct"] if span > MAPPED_SLICE else
                     ["walk-slice", "walk-slice", "staged-slice"]), f
        maps = {"around": rng.choice(np.array(sorted({ngroups - 1, min(ngroups, 255), 255, 0}), dtype=np.uint8), size=span),
                "uniform": mc.draw_map(rng, span, ngroups),
                "one bin": np.full(span, ngroups - 1, dtype=np.uint8),
                "overflow": np.full(span, 255, dtype=np.uint8)}
        for name, codes in maps.items():
            _, _, c, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes,
                                            base, span, ngroups, what=(name, span), every_output=name == "around")
            assert inside.sum() > 1000
            if name == "one bin":
                assert int(c[ngroups - 1]) == int(inside.sum()) and int(c.sum()) == int(c[ngroups - 1])
            if name == "overflow":   # at ngroups = 256 no code reaches the overflow entry
                assert int(c[ngroups]) == (int(inside.sum()) if ngroups < 256 else 0)
                assert int(c[255 if ngroups == 256 else ngroups]) == int(inside.sum())
            if name == "around" and ngroups < 255:
                assert int(c[ngroups]) > 0 and int(c[ngroups - 1]) > 0
            if name == "uniform" and ngroups == 256:
                assert int(c[256]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the knob: the copies of the bins never change a result
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ngroups", (1, 5, 25, 256))
def test_copies_knob(adac, gpu_ctx, ngroups):
    keys, a, b, counts = product_columns()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    rng = np.random.default_rng(86)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    base, span = 1500, 7000
    codes = mc.draw_map(rng, span, ngroups, "skewed")
    d_map = gpu_ctx.upload(padded(codes))
    got = []
    for knob in (0, 1, 4):
        with Knob(adac, "group_mapped_copies", knob, 0):
            check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups,
                          keep, d_mask, (ngroups, knob), every_output=False)
            got.append(run_product(gpu_ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups, d_mask))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 6. every key type against a representative set of (a, b) type pairs: domains at the key type's ends, across zero, one key
# ---------------------------------------------------------------------------------------------------------------------
TYPE_PAIRS = [(np.uint8, np.int64), (np.int32, np.int32), (np.int64, np.uint64), (np.uint16, np.int8),
              (np.uint64, np.uint64)]


@gpu
@pytest.mark.parametrize("atype,btype", TYPE_PAIRS, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ktype", sm.TYPES, ids=lambda t: np.dtype(t).name)
def test_every_key_type(adac, gpu_ctx, ktype, atype, btype):
    keys, a, b = typed_column(ktype), typed_column(atype, side=1), typed_column(btype, side=0)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS_TYPES)
    alay, awords = encode_column(adac, gpu_ctx, a, COUNTS_TYPES)
    blay, bwords = encode_column(adac, gpu_ctx, b, COUNTS_TYPES)
    rng = np.random.default_rng(87)
    keep, d_mask = half_mask(gpu_ctx, rng, COUNTS_TYPES, None, int(klay.value_span))
    rows = 0
    for i, (name, base, span) in enumerate(sm.typed_domains(ktype)):
        ngroups = mc.NGROUPS[i % len(mc.NGROUPS)]
        codes = mc.draw_map(rng, span, ngroups)
        big = span > 1 << 20
        _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, COUNTS_TYPES, codes,
                                        base, span, ngroups, what=(name,), every_output=False)
        if span == 1:
            assert inside.any(), name   # the type's minimum / maximum / -1 are rows of segment 0
        rows += int(inside.sum())
        if not big:
            check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, COUNTS_TYPES, codes, base, span,
                          ngroups, keep, d_mask, (name, "masked"), every_output=False)
    assert rows > 100


# ---------------------------------------------------------------------------------------------------------------------
# 7. segment shapes on each of the three sides: raw, ADAC_NO_MIN, padded, the recompact rule, wrapping frames; then the
#    counts of dense_cases.FUZZ_COUNTS (0, 1, 63 ... 65, 24 577: two scan groups, uneven quarters)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_segment_shapes_on_each_side(adac, gpu_ctx):
    rng = np.random.default_rng(88)
    n = int(COUNTS3.sum())
    plain_a = rng.integers(-900, -100, size=n).astype(np.int16)   # one side of zero: packed against a frame
    plain_b = rng.integers(0, 11, size=n).astype(np.uint8)
    plain_k = (rng.integers(0, 300, size=n) + 70000).astype(np.uint32)
    pa, pb = encode_column(adac, gpu_ctx, plain_a, COUNTS3), encode_column(adac, gpu_ctx, plain_b, COUNTS3)
    pk = encode_column(adac, gpu_ctx, plain_k, COUNTS3)
    met = set()
    for name, (col, rule, pad, check) in kind_columns().items():
        lay, words = encode_column(adac, gpu_ctx, col, COUNTS3, rule=rule, pad=pad)
        assert check(lay.get_descs()), (name, lay.get_descs())
        for want in (64, 1 << 17):   # the column as the keys
            base, span = domain_around(col, want)
            met |= set(product_forms(lay, base, span, pa[0], pb[0]))
            _, _, _, inside = check_product(gpu_ctx, col, plain_a, plain_b, lay, words, pa[0], pa[1], pb[0], pb[1], COUNTS3,
                                            mc.draw_map(rng, span, 9), base, span, 9, what=(name, "keys", want),
                                            every_output=False)
            assert inside.any(), (name, want)
        base, span = 70000 - 5, 290
        met |= set(product_forms(pk[0], base, span, lay, pb[0])) | set(product_forms(pk[0], base, span, pa[0], lay))
        codes = mc.draw_map(rng, span, 2)
        check_product(gpu_ctx, plain_k, col, plain_b, pk[0], pk[1], lay, words, pb[0], pb[1], COUNTS3, codes, base, span, 2,
                      what=(name, "a"), every_output=False)
        check_product(gpu_ctx, plain_k, plain_a, col, pk[0], pk[1], pa[0], pa[1], lay, words, COUNTS3, codes, base, span, 2,
                      what=(name, "b"), every_output=False)
    assert {"staged-direct", "staged-slice", "walk-slice", "walk-direct"} <= met, met
    counts = np.array(dc.FUZZ_COUNTS, dtype=np.uint32)
    nn = int(counts.sum())
    keys = (rng.integers(0, 1 << 12, size=nn) + 5000).astype(np.int32)
    a = rng.integers(0, 1 << 20, size=nn).astype(np.uint32)
    b = rng.integers(-7, 0, size=nn).astype(np.int16)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    for base, span in ((5000 + 100, 1500), (5000 - 20, 3500)):
        f = product_forms(klay, base, span, alay, blay)
        assert f[0] is None and ("walk-slice" if span <= MAPPED_SLICE else "walk-direct") in f, f
        codes = mc.draw_map(rng, span, 7, "mostly255")
        _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base,
                                        span, 7, what=("counts", span))
        assert inside.any()
        check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, 7, keep,
                      d_mask, ("counts", span, "masked"), every_output=False)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the mask: the keys' element space, gaps and the tail set, a and b at other offsets
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ktype,w,span", [(np.int32, 12, 2500), (np.uint16, 3, 5), (np.uint64, 40, 2500)])
def test_mask_geometry(adac, gpu_ctx, ktype, w, span):
    rng = np.random.default_rng(89 + w)
    n = int(COUNTS4.sum())
    keys = (rng.integers(0, 2 ** w, size=n, dtype=np.uint64) + np.uint64(1000)).astype(ktype)
    if w > 16:   # few of 2^w keys would fall into the domain: plant some
        keys[::2] = 1001 + rng.integers(0, span, size=len(keys[::2]), dtype=np.uint64)
    keys[n - 2], keys[n - 1] = 1000, 1000 + 2 ** w - 1
    a = rng.integers(0, 60000, size=n).astype(np.uint16)
    b = rng.integers(-100, 100, size=n).astype(np.int32)
    koffs = gapped_offsets(COUNTS4)
    aoffs = np.array(offsets_of(COUNTS4, None), dtype=np.uint64) + np.uint64(77)
    boffs = np.array(offsets_of(COUNTS4, None), dtype=np.uint64) + np.uint64(131)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS4, koffs)
    alay, awords = encode_column(adac, gpu_ctx, a, COUNTS4, aoffs)
    blay, bwords = encode_column(adac, gpu_ctx, b, COUNTS4, boffs)
    base = 1000 + 1
    keep = rng.random(n) < 0.5
    d_mask = gpu_ctx.upload(dc.full_mask(keep, COUNTS4, [int(o) for o in koffs], int(klay.value_span)))
    codes = mc.draw_map(rng, span, 8)
    _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, COUNTS4, codes, base,
                                    span, 8, keep, d_mask, "gaps")
    assert inside.any() and not keep.all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the map's pad bytes never matter
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("span", (1, 13, MAPPED_SLICE - 3, MAPPED_SLICE + 5, 6001))
def test_map_pad(adac, gpu_ctx, span):
    rng = np.random.default_rng(90)
    counts = np.array([3000, 257], dtype=np.uint32)
    keys = (rng.integers(0, 1 << 13, size=int(counts.sum())) + 500).astype(np.uint32)
    keys[0], keys[1], keys[2] = 500, 500 + (1 << 13) - 1, 700 + span - 1
    keys[3:40] = 700 + rng.integers(0, span, size=37)
    a = rng.integers(0, 1 << 30, size=len(keys)).astype(np.uint32)
    b = rng.integers(1 << 40, 1 << 41, size=len(keys)).astype(np.int64)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    base, ngroups = 700, 4
    codes = mc.draw_map(rng, span, ngroups)
    exp = expected(keys, a, b, codes, base, span, ngroups)
    assert exp[3][2]
    got = []
    for pad in (0, 1, 255):
        check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups,
                      what=(span, pad), every_output=False, pad=pad)
        d_map = gpu_ctx.upload(padded(codes, pad))
        got.append(run_product(gpu_ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(got[0][:3], exp[:3]))


# ---------------------------------------------------------------------------------------------------------------------
# 10. the header form reads nothing: the packed words of its segments overwritten in all three arenas, the map bytes only
#     they could reach garbage, the results stay
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_header_form_reads_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(91)
    counts = np.array([3000, 257, 5000, 1], dtype=np.uint32)
    frames = [1000, 900000, 5000, 2000000]
    keys = np.concatenate([(rng.integers(0, 1 << 12, size=int(c)) + f).astype(np.uint32) for c, f in zip(counts, frames)])
    pos = 0
    for c, f in zip(counts, frames):
        keys[pos], keys[pos + int(c) - 1] = f + (1 << 12) - 1 if c > 1 else f, f
        pos += int(c)
    a = rng.integers(0, 1 << 30, size=len(keys)).astype(np.uint32)
    b = rng.integers(-60, -10, size=len(keys)).astype(np.int8)   # one side of zero: packed against a frame
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    base, span, ngroups = 500, 10000, 6
    f = product_forms(klay, base, span, alay, blay)
    assert f == ["walk-direct", "header", "walk-direct", "header"], f
    codes = mc.draw_map(rng, span, ngroups)
    d_map = gpu_ctx.upload(padded(codes))
    before = run_product(gpu_ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups)
    for lay, words in ((klay, kwords), (alay, awords), (blay, bwords)):
        d = lay.get_descs()
        arena = words.download(np.uint64, int(lay.max_arena_words))
        for s in (1, 3):
            o, nw = int(d["word_off"][s]), (int(d["count"][s]) * int(d["width"][s]) + 63) // 64
            arena[o:o + nw] = POISON
        words.upload(arena)
    # the indices [9096, 10000) are reached by no live segment (the live ones end at 5000 + 4095 - 500 = 8595)
    garbage = codes.copy()
    garbage[9096:] = rng.integers(0, 256, size=span - 9096).astype(np.uint8)
    d_map.upload(padded(garbage, 0x11))
    after = run_product(gpu_ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert int(after[3][1]) == 0 and int(after[3][3]) == 0 and int(after[3][0]) > 0
    exp = expected(keys, a, b, codes, base, span, ngroups)
    assert all(np.array_equal(x, y) for x, y in zip(after[:3], exp[:3]))


# ---------------------------------------------------------------------------------------------------------------------
# 11. aliases: a == b with the same words gives the per-code sum of squares; a == keys
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_aliases(adac, gpu_ctx):
    keys, a, _, counts = product_columns()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    rng = np.random.default_rng(92)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    base, span, ngroups = 1200, 6000, 11
    codes = mc.draw_map(rng, span, ngroups)
    for mask, kp in ((None, None), (d_mask, keep)):
        sab, sa, _, inside = check_product(gpu_ctx, keys, a, a, klay, kwords, alay, awords, alay, awords, counts, codes,
                                           base, span, ngroups, kp, mask, "a == b", every_output=False)
        t, _ = sm.member_index(keys, base, span)
        sq = np.zeros(ngroups + 1, dtype=np.uint64)
        np.add.at(sq, np.minimum(codes[t[inside].astype(np.int64)].astype(np.int64), ngroups),
                  (a[inside].astype(np.int64) ** 2).view(np.uint64))
        assert np.array_equal(sab, sq) and sq[:ngroups].all()
        # a is the key layout itself (staged where the key is 40 bits wide), then b, then both
        check_product(gpu_ctx, keys, keys, a, klay, kwords, klay, kwords, alay, awords, counts, codes, base, span, ngroups,
                      kp, mask, "a == keys", every_output=False)
        check_product(gpu_ctx, keys, a, keys, klay, kwords, alay, awords, klay, kwords, counts, codes, base, span, ngroups,
                      kp, mask, "b == keys", every_output=False)
        check_product(gpu_ctx, keys, keys, keys, klay, kwords, klay, kwords, klay, kwords, counts, codes, base, span,
                      ngroups, kp, mask, "a == b == keys", every_output=False)


# ---------------------------------------------------------------------------------------------------------------------
# 12. cross-oracles on the same columns: adac_scan_group_sum_mapped for SUM(a) and the counts; adac_scan_group_sum_product
#     over the materialised code column codes[t] for SUM(a * b), when every row is inside the domain
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ngroups", (6, 25))
def test_equals_the_older_scans(adac, gpu_ctx, ngroups):
    keys, a, b, counts = product_columns()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    rng = np.random.default_rng(93)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    base, span = 1200, 7000
    codes = mc.draw_map(rng, span, ngroups, "mostly255")
    d_map = gpu_ctx.upload(padded(codes))
    for mask in (None, d_mask):
        ms, mcn, mr = mc.run_sum(gpu_ctx, klay, kwords, alay, awords, d_map, base, span, ngroups, mask)
        sab, sa, c, r = run_product(gpu_ctx, klay, kwords, alay, awords, blay, bwords, d_map, base, span, ngroups, mask)
        assert np.array_equal(sa, ms) and np.array_equal(c, mcn) and np.array_equal(r, mr)
        assert int(c.sum()) > 500 and int(c[ngroups]) > int(c[:ngroups].sum())
    # every row inside the domain: a small key column, its code column materialised with numpy
    n = int(counts.sum())
    keys2 = (rng.integers(0, 3000, size=n) + 40).astype(np.uint16)
    base2, span2 = 40, 3000
    codes2 = mc.draw_map(rng, span2, ngroups)
    code_col = codes2[(keys2 - base2).astype(np.int64)]
    k2, k2w = encode_column(adac, gpu_ctx, keys2, counts)
    cl, clw = encode_column(adac, gpu_ctx, code_col, counts)
    d_map2 = gpu_ctx.upload(padded(codes2))
    nw = ngroups + 1
    d_s, d_c = gpu_ctx.alloc(nw * 8), gpu_ctx.alloc(nw * 8)
    for mask in (None, d_mask):
        alay.scan_group_sum_product(awords, blay, bwords, cl, clw, ngroups, d_s, d_c, mask)
        sab, _, c, r = run_product(gpu_ctx, k2, k2w, alay, awords, blay, bwords, d_map2, base2, span2, ngroups, mask)
        assert np.array_equal(sab, d_s.download(np.uint64, nw)) and np.array_equal(c, d_c.download(np.uint64, nw))
        assert mask is not None or int(r.sum()) == n


# ---------------------------------------------------------------------------------------------------------------------
# 13. the refusals
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors_write_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(94)
    counts = np.array([100, 3000], dtype=np.uint32)
    keys = np.concatenate([sm.segment_at_width(rng, np.int32, int(c), 17) for c in counts])
    a = rng.integers(0, 1000, size=len(keys)).astype(np.uint16)
    b = rng.integers(-5, 5, size=len(keys)).astype(np.int8)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    alay, awords = encode_column(adac, gpu_ctx, a, counts)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts)
    other = encode_column(adac, gpu_ctx, a[:3000], np.array([100, 2900], dtype=np.uint32))
    small = adac.Layout(gpu_ctx, np.uint16, counts)
    ctx2 = adac.Context()
    far = adac.Layout(ctx2, np.uint16, counts)
    nwords = (int(klay.value_span) + 63) // 64
    span, ng = 100, 9
    mwords = mc.map_bytes(span) // 8
    d_ab, d_a, d_c, d_r = (gpu_ctx.alloc((ng + 1) * 8), gpu_ctx.alloc((ng + 1) * 8), gpu_ctx.alloc((ng + 1) * 8),
                           gpu_ctx.alloc(2 * 8))
    d_mask = gpu_ctx.upload(np.full(nwords, POISON, dtype=np.uint64))
    d_map = gpu_ctx.upload(np.full(mwords, POISON, dtype=np.uint64))
    bufs = ((d_ab, ng + 1), (d_a, ng + 1), (d_c, ng + 1), (d_r, 2), (d_mask, nwords), (d_map, mwords))
    for buf, nw in bufs[:4]:
        buf.upload(np.full(nw, POISON, dtype=np.uint64))
    pm = klay.scan_group_sum_product_mapped
    i32max = 0x7FFFFFFF

    def call(kw=kwords, al=alay, aw=awords, bl=blay, bw=bwords, m=d_map, base=0, sp=span, n=ng, ab=d_ab, sa=d_a, c=d_c,
             r=d_r, mask=None, on=pm):
        return lambda: on(kw, al, aw, bl, bw, m, base, sp, n, ab, sa, c, r, mask)
    last = 8 * ng
    refused = [
        # key_span outside 1 ... 2^32, a domain that leaves the type
        call(sp=0), call(base=1 << 31, sp=(1 << 32) + 1), call(base=i32max, sp=2), call(base=i32max - 9, sp=11),
        call(base=1 << 32, sp=10), call(base=1 << 40, sp=10),
        call(on=small.scan_group_sum_product_mapped, base=65530, sp=7),
        # ngroups outside 1 ... 256
        call(n=0), call(n=257),
        # a NULL map, a map that is not 8-byte aligned
        call(m=None), call(m=d_map.ptr + 4, sp=span - 8), call(m=d_map.ptr + 1, sp=span - 8),
        # NULL d_sums_ab; NULL words of each column; words not 16-byte aligned
        call(ab=None), call(kw=None), call(aw=None), call(bw=None),
        call(kw=kwords.ptr + 8), call(aw=awords.ptr + 8), call(bw=bwords.ptr + 8),
        # per-segment counts that differ between any two of the three, layouts on different contexts
        call(al=other[0], aw=other[1]), call(bl=other[0], bw=other[1]),
        call(al=other[0], aw=other[1], bl=other[0], bw=other[1]),
        call(al=far), call(bl=far),
        # any two of the outputs and the mask overlapping
        call(sa=d_ab), call(c=d_ab), call(r=d_ab), call(c=d_a), call(r=d_a), call(r=d_c),
        call(sa=d_ab.ptr + last), call(c=d_a.ptr + last), call(r=d_c.ptr + last), call(c=d_ab.ptr + last),
        call(ab=d_mask, mask=d_mask), call(sa=d_mask, mask=d_mask), call(c=d_mask, mask=d_mask),
        call(r=d_mask.ptr + 8 * (nwords - 1), mask=d_mask),
        # the map overlapping an output
        call(ab=d_map), call(sa=d_map), call(c=d_map.ptr + 8 * (mwords - 1)), call(r=d_map.ptr + 8 * (mwords - 1)),
    ]
    for i, refused_call in enumerate(refused):
        with pytest.raises(adac.AdacError) as e:
            refused_call()
        assert e.value.status == INVALID_ARGUMENT, i
    L = adac.lib()
    for handles in ((None, alay._h, blay._h), (klay._h, None, blay._h), (klay._h, alay._h, None)):   # a NULL layout
        assert L.adac_scan_group_sum_product_mapped(handles[0], kwords.ptr, handles[1], awords.ptr, handles[2], bwords.ptr,
                                                    None, d_map.ptr, 0, span, ng, d_ab.ptr, d_a.ptr, d_c.ptr,
                                                    d_r.ptr) == INVALID_ARGUMENT
    gpu_ctx.sync()
    for buf, nw in bufs:
        assert (buf.download(np.uint64, nw) == POISON).all()
    # a key layout without segments: ADAC_OK, the outputs that were given zero-filled
    e1 = adac.Layout(gpu_ctx, np.int32, np.zeros(0, np.uint32))
    ea, eb = adac.Layout(gpu_ctx, np.uint16, np.zeros(0, np.uint32)), adac.Layout(gpu_ctx, np.int8, np.zeros(0, np.uint32))
    e1.scan_group_sum_product_mapped(None, ea, None, eb, None, d_map, 1 << 31, span, ng, d_ab, d_a, None, None)
    assert not d_ab.download(np.uint64, ng + 1).any() and not d_a.download(np.uint64, ng + 1).any()
    assert (d_c.download(np.uint64, ng + 1) == POISON).all()
    d_ab.upload(np.full(ng + 1, POISON, dtype=np.uint64))
    e1.scan_group_sum_product_mapped(None, ea, None, eb, None, d_map, 1 << 31, span, ng, d_ab, None, d_c, None)
    assert not d_ab.download(np.uint64, ng + 1).any() and not d_c.download(np.uint64, ng + 1).any()
    # segments without rows only: everything written, nothing counted
    z = [adac.Layout(gpu_ctx, t, np.zeros(2, np.uint32)) for t in (np.int32, np.uint16, np.int8)]
    for buf, nw in bufs[:4]:
        buf.upload(np.full(nw, POISON, dtype=np.uint64))
    z[0].scan_group_sum_product_mapped(None, z[1], None, z[2], None, d_map, 0, span, ng, d_ab, d_a, d_c, d_r)
    assert d_r.download(np.uint64, 2).tolist() == [0, 0]
    assert not any(buf.download(np.uint64, ng + 1).any() for buf in (d_ab, d_a, d_c))
    # after the refusals the codec is still usable
    base, span2 = domain_around(keys, 1 << 16)
    _, _, _, inside = check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts,
                                    mc.draw_map(rng, span2, ng), base, span2, ng, what="afterwards")
    assert inside.any()
    far.close()
    ctx2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 14. Q5-shaped: a map built from an orders-like table under a date bitmap, the revenue of a lineitem-like table through it
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_q5_revenue_round_trip(adac, gpu_ctx):
    rng = np.random.default_rng(95)
    n_orders, nations = 50_000, 25
    o_orderkey = sparse_keys(n_orders).astype(np.int32)
    o_nation = rng.integers(0, nations, size=n_orders).astype(np.uint8)   # the nation of the order's customer
    o_orderdate = rng.integers(8000, 10600, size=n_orders).astype(np.int32)
    per = rng.integers(1, 8, size=n_orders)
    l_orderkey = np.repeat(o_orderkey, per)
    n_items = len(l_orderkey)
    l_price = rng.integers(90000, 10500000, size=n_items).astype(np.int64)
    l_disc = rng.integers(0, 11, size=n_items).astype(np.int8)
    oc, lc = segments_of(n_orders), segments_of(n_items)
    okey, onat = encode_column(adac, gpu_ctx, o_orderkey, oc), encode_column(adac, gpu_ctx, o_nation, oc)
    odate = encode_column(adac, gpu_ctx, o_orderdate, oc)
    lkey, price = encode_column(adac, gpu_ctx, l_orderkey, lc), encode_column(adac, gpu_ctx, l_price, lc)
    disc = encode_column(adac, gpu_ctx, l_disc, lc)
    # WHERE o_orderdate >= 8766 AND o_orderdate < 9131, as a bitmap over the orders
    ow = (n_orders + 63) // 64
    d_obm, d_ocnt = gpu_ctx.alloc(ow * 8), gpu_ctx.alloc(len(oc) * 8)
    odate[0].scan_select_between(odate[1], 8766, 9130, d_obm, d_ocnt)
    year = (o_orderdate >= 8766) & (o_orderdate <= 9130)
    assert 0.05 < year.mean() < 0.5
    base, span = 1, int(o_orderkey.max())
    d_map = gpu_ctx.alloc(mc.map_bytes(span))
    okey[0].scan_build_map(okey[1], onat[0], onat[1], base, span, d_map, 255, None, d_obm)
    exp_map = np.full(mc.map_bytes(span), 255, dtype=np.uint8)
    exp_map[(o_orderkey[year] - base).astype(np.int64)] = o_nation[year]
    assert np.array_equal(d_map.download(np.uint8, mc.map_bytes(span)), exp_map)
    assert set(product_forms(lkey[0], base, span, price[0], disc[0])) == {"walk-direct"}
    sab, sa, c, r = run_product(gpu_ctx, lkey[0], lkey[1], price[0], price[1], disc[0], disc[1], d_map, base, span, nations)
    g = np.minimum(exp_map[(l_orderkey - base).astype(np.int64)].astype(np.int64), nations)
    exp_rev, exp_c = np.zeros(nations + 1, dtype=np.uint64), np.zeros(nations + 1, dtype=np.uint64)
    np.add.at(exp_rev, g, (l_price * (100 - l_disc.astype(np.int64))).view(np.uint64))   # SUM(price * (100 - disc))
    np.add.at(exp_c, g, np.uint64(1))
    assert np.array_equal(np.uint64(100) * sa - sab, exp_rev) and np.array_equal(c, exp_c)
    assert int(c[nations]) > int(c[:nations].sum()) > 0   # most rows are dropped by the filter, some are not
    assert int(r.sum()) == n_items
