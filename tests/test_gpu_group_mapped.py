"""adac_scan_group_sum_mapped / adac_scan_group_count_mapped / adac_scan_build_map: SUM(value), COUNT(*) GROUP BY a code
looked up through a dense key, on the packed bytes of both columns, and the scan that builds the map.  Expected values
are numpy over the ORIGINAL columns (mapped_cases.expected / built_map).  Every call is made twice into poisoned outputs
with one spare word after each, which must stay poison, and the two results must be equal."""
import numpy as np
import pytest

import dense_cases as dc
import mapped_cases as mc
import scan_member_cases as sm
from mapped_cases import ALL_FORMS, MAPPED_SLICE, check_build, check_mapped, expected, mapped_forms, padded, run_count, run_sum
from scan_member_cases import POISON
from scan_compare_cases import typed_column, COUNTS_TYPES
from test_gpu_group_dense import Knob, domain_around, segments_of
from test_gpu_scan_select_compare import COUNTS4, gapped_offsets, half_mask
from test_gpu_sum_product import COUNTS3, encode_column, kind_columns, offsets_of

gpu = pytest.mark.gpu
INVALID_ARGUMENT = 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. every key width, each segment with a domain of its own inside its interval; caps on both sides of MAPPED_SLICE
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", sm.GRID_TYPES, ids=lambda t: np.dtype(t).name)
def test_key_width_grid(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    keys, vals, doms = mc.key_width_grid(dtype)
    nseg = 8 * dtype.itemsize
    counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    assert [int(w) for w in klay.get_descs()["width"]] == list(range(1, nseg + 1))
    assert len(set(int(w) for w in vlay.get_descs()["width"])) == 16
    rng = np.random.default_rng(61)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    seen = set()
    for s, (base, span) in enumerate(doms):
        f = mapped_forms(klay, base, span, vlay)
        assert f[s] not in (None, "header")
        assert f[s].endswith("-slice") == (span <= MAPPED_SLICE), (s + 1, f[s], span)
        seen |= set(f) | set(mapped_forms(klay, base, span))
        ngroups = mc.NGROUPS[s % len(mc.NGROUPS)]
        codes = mc.draw_map(rng, span, ngroups)
        _, _, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups,
                                    what=(s + 1,))
        mine = inside[s * sm.ROWS_GRID:(s + 1) * sm.ROWS_GRID]
        assert mine.any() and (s == 0 or not mine.all()), s + 1   # rows inside and outside the domain
        check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups, keep, d_mask,
                     (s + 1, "masked"), every_entry=False)
    # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 indices: no staged reader without a slice)
    assert seen >= ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. ngroups and the maps around it; one bin for every row; the overflow entry for every row; no overflow at 256
# ---------------------------------------------------------------------------------------------------------------------
def ngroups_column():
    """two segments past a scan group (walk, slice and direct by the domain) and one at w = 40 (staged)"""
    rng = np.random.default_rng(62)
    counts = np.array([24577, 4099, 1000], dtype=np.uint32)
    keys = np.concatenate([rng.integers(0, 1 << 13, size=int(counts[0])) + 1000,
                           rng.integers(0, 1 << 13, size=int(counts[1])) + 3000,
                           rng.integers(0, 1 << 40, size=int(counts[2]))]).astype(np.uint64)
    keys[0], keys[1] = 1000, 1000 + (1 << 13) - 1
    keys[-300:] = rng.integers(1000, 9000, size=300)
    keys[-301] = (1 << 40) - 1
    vals = rng.integers(-(1 << 20), -5, size=len(keys)).astype(np.int32)   # negative, packed against a frame
    return keys, vals, counts


@gpu
@pytest.mark.parametrize("ngroups", mc.NGROUPS)
def test_ngroups(adac, gpu_ctx, ngroups):
    keys, vals, counts = ngroups_column()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    rng = np.random.default_rng(63 + ngroups)
    for base, span in ((1000 + 5, 8000), (2000, MAPPED_SLICE - 7)):
        f = mapped_forms(klay, base, span, vlay)
        assert f == (["walk-direct", "walk-direct", "staged-direct"] if span > MAPPED_SLICE else
                     ["walk-slice", "walk-slice", "staged-slice"]), f
        maps = {"around": rng.choice(np.array(sorted({ngroups - 1, min(ngroups, 255), 255, 0}), dtype=np.uint8), size=span),
                "uniform": mc.draw_map(rng, span, ngroups),
                "one bin": np.full(span, ngroups - 1, dtype=np.uint8),
                "overflow": np.full(span, 255, dtype=np.uint8)}
        for name, codes in maps.items():
            s, c, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups,
                                        what=(name, span), every_entry=name == "around")
            assert inside.sum() > 1000
            if name == "one bin":
                assert int(c[ngroups - 1]) == int(inside.sum()) and int(c.sum()) == int(c[ngroups - 1])
            if name == "overflow":   # at ngroups = 256 no code reaches the overflow entry
                assert int(c[ngroups]) == (int(inside.sum()) if ngroups < 256 else 0)
                assert int(c[255 if ngroups == 256 else ngroups]) == int(inside.sum())
            if name == "around" and ngroups < 255:
                assert int(c[ngroups]) > 0 and int(c[ngroups - 1]) > 0
        if ngroups == 256:
            assert int(check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, maps["uniform"], base, span,
                                    256, what="256")[1][256]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the knob: the copies of the bins never change a result
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ngroups", (1, 5, 25, 256))
def test_copies_knob(adac, gpu_ctx, ngroups):
    keys, vals, counts = ngroups_column()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    rng = np.random.default_rng(64)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    base, span = 1500, 7000
    codes = mc.draw_map(rng, span, ngroups, "skewed")
    d_map = gpu_ctx.upload(padded(codes))
    got = []
    for knob in (0, 1, 4):
        with Knob(adac, "group_mapped_copies", knob, 0):
            check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups, keep, d_mask,
                         (ngroups, knob))
            got.append(run_sum(gpu_ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups, d_mask))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 4. every value width of the 8-byte types against a key at w = 13; sums that wrap, negative values
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("vtype", [np.uint64, np.int64], ids=lambda t: np.dtype(t).name)
def test_value_widths(adac, gpu_ctx, vtype):
    vtype = np.dtype(vtype)
    rng = np.random.default_rng(65 + vtype.itemsize + (vtype.kind == "i"))
    rows, nseg = 257, 64
    counts = np.full(nseg, rows, dtype=np.uint32)
    keys = (1000 + rng.integers(200, 4000, size=rows * nseg)).astype(np.uint32)
    keys[rng.random(rows * nseg) < 0.2] = 1000 + 7000   # outside the domains below
    keys[0::rows], keys[1::rows] = 1000, 1000 + (1 << 13) - 1
    vals = np.concatenate([sm.segment_at_width(rng, vtype, rows, w) for w in range(1, 65)])
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    assert all(int(w) == 13 for w in klay.get_descs()["width"])
    assert [int(w) for w in vlay.get_descs()["width"]] == list(range(1, 65))
    ngroups = 3
    for base, span, acc in ((1000 + 200, MAPPED_SLICE, "slice"), (1100, 5000, "direct")):
        f = mapped_forms(klay, base, span, vlay)
        assert f == ["walk-" + acc] * 32 + ["staged-" + acc] * 32, f   # widths above 32 fall to the staged reader
        codes = mc.draw_map(rng, span, ngroups)
        s, c, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups,
                                    what=(acc,))
        assert inside.sum() > 200
    t, _ = sm.member_index(keys, base, span)
    exact = [0] * (ngroups + 1)
    for i in np.nonzero(inside)[0]:
        exact[min(int(codes[int(t[i])]), ngroups)] += int(vals[i])
    if vtype.kind == "u":
        assert any(x >= 2 ** 64 for x in exact), "no sum wrapped"
    else:
        assert (vals[inside] < 0).any() and (vals[inside] > 0).any()
    assert [int(x) for x in s] == [x % 2 ** 64 for x in exact]


# ---------------------------------------------------------------------------------------------------------------------
# 5. every type pair: domains at the key type's ends, across zero, one key, 2^24 keys
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("vtype", dc.VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ktype", sm.TYPES, ids=lambda t: np.dtype(t).name)
def test_every_type_pair(adac, gpu_ctx, ktype, vtype):
    keys, vals = typed_column(ktype), typed_column(vtype, side=1)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS_TYPES)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, COUNTS_TYPES)
    rng = np.random.default_rng(66)
    keep, d_mask = half_mask(gpu_ctx, rng, COUNTS_TYPES, None, int(klay.value_span))
    rows = 0
    for i, (name, base, span) in enumerate(sm.typed_domains(ktype)):
        ngroups = mc.NGROUPS[i % len(mc.NGROUPS)]
        codes = mc.draw_map(rng, span, ngroups)
        big = span > 1 << 20
        _, c, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS_TYPES, codes, base, span,
                                    ngroups, what=(name,), every_entry=not big)
        if span == 1:
            assert inside.any(), name   # the type's minimum / maximum / -1 are rows of segment 0
        rows += int(inside.sum())
        if not big:
            check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS_TYPES, codes, base, span, ngroups, keep,
                         d_mask, (name, "masked"), every_entry=False)
    assert rows > 100


# ---------------------------------------------------------------------------------------------------------------------
# 6. segment shapes on either side: raw, ADAC_NO_MIN, padded, the recompact rule, wrapping frames; then the counts of
#    dense_cases.FUZZ_COUNTS (0, 1, 63 ... 65, 24 577: two scan groups, uneven quarters)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_segment_shapes_on_either_side(adac, gpu_ctx):
    rng = np.random.default_rng(67)
    n = int(COUNTS3.sum())
    plain_v = rng.integers(-900, -100, size=n).astype(np.int16)   # one side of zero: packed against a frame
    plain_k = (rng.integers(0, 300, size=n) + 70000).astype(np.uint32)
    pv, pk = encode_column(adac, gpu_ctx, plain_v, COUNTS3), encode_column(adac, gpu_ctx, plain_k, COUNTS3)
    met = set()
    for name, (col, rule, pad, check) in kind_columns().items():
        lay, words = encode_column(adac, gpu_ctx, col, COUNTS3, rule=rule, pad=pad)
        assert check(lay.get_descs()), (name, lay.get_descs())
        for want in (64, 1 << 17):   # the column as the keys
            base, span = domain_around(col, want)
            met |= set(mapped_forms(lay, base, span, pv[0]))
            _, _, inside = check_mapped(gpu_ctx, col, plain_v, lay, words, pv[0], pv[1], COUNTS3, mc.draw_map(rng, span, 9),
                                        base, span, 9, what=(name, "keys", want))
            assert inside.any(), (name, want)
        base, span = 70000 - 5, 290   # the column as the values
        met |= set(mapped_forms(pk[0], base, span, lay))
        check_mapped(gpu_ctx, plain_k, col, pk[0], pk[1], lay, words, COUNTS3, mc.draw_map(rng, span, 2), base, span, 2,
                     what=(name, "values"), every_entry=False)
    assert {"staged-direct", "staged-slice", "walk-slice", "walk-direct"} <= met, met
    counts = np.array(dc.FUZZ_COUNTS, dtype=np.uint32)
    nn = int(counts.sum())
    keys = (rng.integers(0, 1 << 12, size=nn) + 5000).astype(np.int32)
    vals = rng.integers(0, 1 << 20, size=nn).astype(np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    for base, span in ((5000 + 100, 1500), (5000 - 20, 3500)):
        f = mapped_forms(klay, base, span, vlay)
        assert f[0] is None and ("walk-slice" if span <= MAPPED_SLICE else "walk-direct") in f, f
        codes = mc.draw_map(rng, span, 7, "mostly255")
        _, _, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, 7,
                                    what=("counts", span))
        assert inside.any()
        check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, 7, keep, d_mask,
                     ("counts", span, "masked"), every_entry=False)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the mask: the keys' element space, gaps and the tail set, the values at other offsets
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ktype,w,span", [(np.int32, 12, 2500), (np.uint16, 3, 5), (np.uint64, 40, 2500)])
def test_mask_geometry(adac, gpu_ctx, ktype, w, span):
    rng = np.random.default_rng(68 + w)
    n = int(COUNTS4.sum())
    keys = (rng.integers(0, 2 ** w, size=n, dtype=np.uint64) + np.uint64(1000)).astype(ktype)
    if w > 16:   # few of 2^w keys would fall into the domain: plant some
        keys[::2] = 1001 + rng.integers(0, span, size=len(keys[::2]), dtype=np.uint64)
    keys[n - 2], keys[n - 1] = 1000, 1000 + 2 ** w - 1
    vals = rng.integers(0, 60000, size=n).astype(np.uint16)
    koffs = gapped_offsets(COUNTS4)
    voffs = np.array(offsets_of(COUNTS4, None), dtype=np.uint64) + np.uint64(77)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS4, koffs)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, COUNTS4, voffs)
    base = 1000 + 1
    keep = rng.random(n) < 0.5
    d_mask = gpu_ctx.upload(dc.full_mask(keep, COUNTS4, [int(o) for o in koffs], int(klay.value_span)))
    codes = mc.draw_map(rng, span, 8)
    _, _, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS4, codes, base, span, 8, keep,
                                d_mask, "gaps")
    assert inside.any() and not keep.all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the map's pad bytes, and the bytes past key_span of a longer map, never matter
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("span", (1, 13, MAPPED_SLICE - 3, MAPPED_SLICE + 5, 6001))
def test_map_pad(adac, gpu_ctx, span):
    rng = np.random.default_rng(69)
    counts = np.array([3000, 257], dtype=np.uint32)
    keys = (rng.integers(0, 1 << 13, size=int(counts.sum())) + 500).astype(np.uint32)
    keys[0], keys[1], keys[2] = 500, 500 + (1 << 13) - 1, 700 + span - 1
    keys[3:40] = 700 + rng.integers(0, span, size=37)
    vals = rng.integers(0, 1 << 30, size=len(keys)).astype(np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    base, ngroups = 700, 4
    codes = mc.draw_map(rng, span, ngroups)
    exp_s, exp_c, inside = expected(keys, vals, codes, base, span, ngroups)
    assert inside[2]
    got = []
    for pad in (0, 1, 255):
        check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups, what=(span, pad),
                     pad=pad)
        d_map = gpu_ctx.upload(padded(codes, pad))
        got.append(run_sum(gpu_ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert np.array_equal(x, y)
    assert np.array_equal(got[0][0], exp_s) and np.array_equal(got[0][1], exp_c)


# ---------------------------------------------------------------------------------------------------------------------
# 9. the header form reads nothing: the packed words of its segments overwritten, the map bytes only they could reach
#    garbage, the results stay
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_header_form_reads_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(70)
    counts = np.array([3000, 257, 5000, 1], dtype=np.uint32)
    frames = [1000, 900000, 5000, 2000000]
    keys = np.concatenate([(rng.integers(0, 1 << 12, size=int(c)) + f).astype(np.uint32) for c, f in zip(counts, frames)])
    pos = 0
    for c, f in zip(counts, frames):
        keys[pos], keys[pos + int(c) - 1] = f + (1 << 12) - 1 if c > 1 else f, f
        pos += int(c)
    vals = rng.integers(0, 1 << 30, size=len(keys)).astype(np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    base, span, ngroups = 500, 10000, 6
    f = mapped_forms(klay, base, span, vlay)
    assert f == ["walk-direct", "header", "walk-direct", "header"], f
    codes = mc.draw_map(rng, span, ngroups)
    d_map = gpu_ctx.upload(padded(codes))
    before = run_sum(gpu_ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups)
    before_c = run_count(gpu_ctx, klay, kwords, d_map, base, span, ngroups)
    for lay, words in ((klay, kwords), (vlay, vwords)):
        d = lay.get_descs()
        arena = words.download(np.uint64, int(lay.max_arena_words))
        for s in (1, 3):
            o, nw = int(d["word_off"][s]), (int(d["count"][s]) * int(d["width"][s]) + 63) // 64
            arena[o:o + nw] = POISON
        words.upload(arena)
    # a second domain that the header segments' intervals would fall into if their words were read as garbage: the
    # indices [9096, 10000) are reached by no live segment (the live ones end at 5000 + 4095 - 500 = 8595)
    garbage = codes.copy()
    garbage[9096:] = rng.integers(0, 256, size=span - 9096).astype(np.uint8)
    d_map.upload(padded(garbage, 0x11))
    after = run_sum(gpu_ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups)
    after_c = run_count(gpu_ctx, klay, kwords, d_map, base, span, ngroups)
    for x, y in list(zip(before, after)) + list(zip(before_c, after_c)):
        assert np.array_equal(x, y)
    assert int(after[2][1]) == 0 and int(after[2][3]) == 0 and int(after[2][0]) > 0
    exp_s, exp_c, _ = expected(keys, vals, codes, base, span, ngroups)
    assert np.array_equal(after[0], exp_s) and np.array_equal(after[1], exp_c)


# ---------------------------------------------------------------------------------------------------------------------
# 10. cross-oracle: the fold of adac_scan_group_sum_dense's outputs through the map, on the same columns
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("span", (400, 7000))
def test_equals_the_dense_scan_folded_through_the_map(adac, gpu_ctx, span):
    keys, vals, counts = ngroups_column()
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    rng = np.random.default_rng(71)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    base, ngroups = 1200, 25
    codes = mc.draw_map(rng, span, ngroups, "mostly255" if span > 1000 else "uniform")
    d_map = gpu_ctx.upload(padded(codes))
    for mask in (None, d_mask):
        ds, dcn, dr = dc.run_sum(gpu_ctx, klay, kwords, vlay, vwords, base, span, mask)
        g = np.minimum(codes.astype(np.int64), ngroups)
        fold_s, fold_c = np.zeros(ngroups + 1, dtype=np.uint64), np.zeros(ngroups + 1, dtype=np.uint64)
        np.add.at(fold_s, g, ds)
        np.add.at(fold_c, g, dcn)
        s, c, r = run_sum(gpu_ctx, klay, kwords, vlay, vwords, d_map, base, span, ngroups, mask)
        assert np.array_equal(s, fold_s) and np.array_equal(c, fold_c) and np.array_equal(r, dr)
        assert int(c.sum()) > 500


# ---------------------------------------------------------------------------------------------------------------------
# 11. the refusals
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors_write_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(72)
    counts = np.array([100, 3000], dtype=np.uint32)
    keys = np.concatenate([sm.segment_at_width(rng, np.int32, int(c), 17) for c in counts])
    vals = rng.integers(0, 1000, size=len(keys)).astype(np.uint16)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    other = encode_column(adac, gpu_ctx, vals[:3000], np.array([100, 2900], dtype=np.uint32))
    small = adac.Layout(gpu_ctx, np.uint16, counts)
    ctx2 = adac.Context()
    far = adac.Layout(ctx2, np.uint16, counts)
    nwords = (int(klay.value_span) + 63) // 64
    span, ng = 100, 9
    mwords = mc.map_bytes(span) // 8
    d_s, d_c, d_r = gpu_ctx.alloc((ng + 1) * 8), gpu_ctx.alloc((ng + 1) * 8), gpu_ctx.alloc(2 * 8)
    d_mask = gpu_ctx.upload(np.full(nwords, POISON, dtype=np.uint64))
    d_map = gpu_ctx.upload(np.full(mwords, POISON, dtype=np.uint64))
    bufs = ((d_s, ng + 1), (d_c, ng + 1), (d_r, 2), (d_mask, nwords), (d_map, mwords))
    for b, nw in bufs[:3]:
        b.upload(np.full(nw, POISON, dtype=np.uint64))
    sm_, cn_, bm_ = klay.scan_group_sum_mapped, klay.scan_group_count_mapped, klay.scan_build_map
    i32max = 0x7FFFFFFF
    refused = [
        # key_span outside 1 ... 2^32, a domain that leaves the type
        lambda: sm_(kwords, vlay, vwords, d_map, 0, 0, ng, d_s, d_c, d_r), lambda: cn_(kwords, d_map, 0, 0, ng, d_c, d_r),
        lambda: bm_(kwords, vlay, vwords, 0, 0, d_map),
        lambda: sm_(kwords, vlay, vwords, d_map, 1 << 31, (1 << 32) + 1, ng, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, i32max, 2, ng, d_s, d_c, d_r),
        lambda: cn_(kwords, d_map, i32max - 9, 11, ng, d_c, d_r), lambda: bm_(kwords, vlay, vwords, i32max - 9, 11, d_map),
        lambda: sm_(kwords, vlay, vwords, d_map, 1 << 32, 10, ng, d_s, d_c, d_r),
        lambda: cn_(kwords, d_map, 1 << 40, 10, ng, d_c, d_r), lambda: bm_(kwords, vlay, vwords, 1 << 40, 10, d_map),
        lambda: small.scan_group_count_mapped(kwords, d_map, 65530, 7, ng, d_c, d_r),
        # ngroups outside 1 ... 256, fill above 255
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, 0, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, 257, d_s, d_c, d_r),
        lambda: cn_(kwords, d_map, 0, span, 0, d_c, d_r), lambda: cn_(kwords, d_map, 0, span, 257, d_c, d_r),
        lambda: bm_(kwords, vlay, vwords, 0, span, d_map, 256),
        # a NULL map, a map that is not 8-byte aligned
        lambda: sm_(kwords, vlay, vwords, None, 0, span, ng, d_s, d_c, d_r), lambda: cn_(kwords, None, 0, span, ng, d_c, d_r),
        lambda: bm_(kwords, vlay, vwords, 0, span, None),
        lambda: sm_(kwords, vlay, vwords, d_map.ptr + 4, 0, span - 8, ng, d_s, d_c, d_r),
        lambda: cn_(kwords, d_map.ptr + 1, 0, span - 8, ng, d_c, d_r),
        lambda: bm_(kwords, vlay, vwords, 0, span - 8, d_map.ptr + 4),
        # a required output that is NULL; NULL words; words not 16-byte aligned
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, None, d_c, d_r),
        lambda: cn_(kwords, d_map, 0, span, ng, None, d_r),
        lambda: sm_(None, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, None, d_map, 0, span, ng, d_s, d_c, d_r),
        lambda: cn_(None, d_map, 0, span, ng, d_c, d_r), lambda: bm_(None, vlay, vwords, 0, span, d_map),
        lambda: bm_(kwords, vlay, None, 0, span, d_map),
        lambda: sm_(kwords.ptr + 8, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords.ptr + 8, d_map, 0, span, ng, d_s, d_c, d_r),
        lambda: cn_(kwords.ptr + 8, d_map, 0, span, ng, d_c, d_r), lambda: bm_(kwords, vlay, vwords.ptr + 8, 0, span, d_map),
        # per-segment counts that differ, layouts on different contexts
        lambda: sm_(kwords, other[0], other[1], d_map, 0, span, ng, d_s, d_c, d_r),
        lambda: bm_(kwords, other[0], other[1], 0, span, d_map),
        lambda: sm_(kwords, far, vwords, d_map, 0, span, ng, d_s, d_c, d_r), lambda: bm_(kwords, far, vwords, 0, span, d_map),
        # any two of the outputs and the mask overlapping
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_s, d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_s),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_s.ptr + 8 * ng, d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_c.ptr + 8 * ng),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_mask, d_c, d_r, d_mask),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_mask, d_r, d_mask),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_mask.ptr + 8 * (nwords - 1), d_mask),
        lambda: cn_(kwords, d_map, 0, span, ng, d_c, d_c), lambda: cn_(kwords, d_map, 0, span, ng, d_mask, d_r, d_mask),
        # the map overlapping an output; for the build the map overlapping the rows per segment or the mask
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_map, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_map.ptr + 8 * (mwords - 1), d_r),
        lambda: sm_(kwords, vlay, vwords, d_map, 0, span, ng, d_s, d_c, d_map.ptr + 8 * (mwords - 1)),
        lambda: cn_(kwords, d_map, 0, span, ng, d_map, d_r), lambda: cn_(kwords, d_map, 0, span, ng, d_c, d_map),
        lambda: bm_(kwords, vlay, vwords, 0, span, d_map, 255, d_map.ptr + 8 * (mwords - 1)),
        lambda: bm_(kwords, vlay, vwords, 0, span, d_mask, 255, None, d_mask),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(adac.AdacError) as e:
            call()
        assert e.value.status == INVALID_ARGUMENT, i
    with pytest.raises(Exception):
        klay.scan_group_sum_mapped(kwords, None, vwords, d_map, 0, span, ng, d_s, d_c, d_r)   # a NULL value layout
    L = adac.lib()
    assert L.adac_scan_group_sum_mapped(klay._h, kwords.ptr, None, vwords.ptr, None, d_map.ptr, 0, span, ng, d_s.ptr,
                                        d_c.ptr, d_r.ptr) == INVALID_ARGUMENT
    assert L.adac_scan_build_map(klay._h, kwords.ptr, None, vwords.ptr, None, 0, span, 255, d_map.ptr,
                                 None) == INVALID_ARGUMENT
    gpu_ctx.sync()
    for b, nw in bufs:
        assert (b.download(np.uint64, nw) == POISON).all()
    # a key layout without segments: ADAC_OK, the outputs zero-filled, the build's map filled
    e1, ev = adac.Layout(gpu_ctx, np.int32, np.zeros(0, np.uint32)), adac.Layout(gpu_ctx, np.uint16, np.zeros(0, np.uint32))
    e1.scan_group_sum_mapped(None, ev, None, d_map, 1 << 31, span, ng, d_s, d_c, None)
    assert not d_s.download(np.uint64, ng + 1).any() and not d_c.download(np.uint64, ng + 1).any()
    d_c.upload(np.full(ng + 1, POISON, dtype=np.uint64))
    e1.scan_group_count_mapped(None, d_map, 1 << 31, span, ng, d_c, None)
    assert not d_c.download(np.uint64, ng + 1).any()
    e1.scan_build_map(None, ev, None, 1 << 31, span, d_map, 7)
    assert (d_map.download(np.uint8, mwords * 8) == 7).all()
    # segments without rows only: everything written, nothing counted
    z1 = adac.Layout(gpu_ctx, np.int32, np.zeros(2, np.uint32))
    d_r.upload(np.full(2, POISON, dtype=np.uint64))
    z1.scan_group_count_mapped(None, d_map, 0, span, ng, d_c, d_r)
    assert d_r.download(np.uint64, 2).tolist() == [0, 0] and not d_c.download(np.uint64, ng + 1).any()
    # after the refusals the codec is still usable
    base, span2 = domain_around(keys, 1 << 16)
    _, _, inside = check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, mc.draw_map(rng, span2, ng), base,
                                span2, ng, what="afterwards")
    assert inside.any()
    # the largest legal domain: the build over one that ends exactly at the key type's maximum is not refused
    check_build(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, i32max - 10, 11, 255, what="up to the type's maximum")
    far.close()
    ctx2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 12. the build: sparse distinct keys, the mask, rows outside the domain, codes above 255, fill, pad, duplicates
# ---------------------------------------------------------------------------------------------------------------------
def sparse_keys(n):
    idx = np.arange(n, dtype=np.int64)
    return (idx // 8) * 32 + idx % 8 + 1   # sparse-increasing, as dbgen's o_orderkey


@gpu
@pytest.mark.parametrize("ctype", (np.uint8, np.int8, np.uint16, np.int32, np.uint64), ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("fill", (0, 255))
def test_build(adac, gpu_ctx, ctype, fill):
    ctype = np.dtype(ctype)
    rng = np.random.default_rng(73 + ctype.itemsize)
    counts = np.array([24577, 0, 1, 65, 4099], dtype=np.uint32)
    n = int(counts.sum())
    keys = sparse_keys(n).astype(np.int32)
    hi = min(int(np.iinfo(ctype).max), 400)
    codes = rng.integers(0, hi, size=n, endpoint=True).astype(ctype)   # codes above 255 saturate (wide types)
    if ctype.kind == "i":
        codes[::7] = -1 - rng.integers(0, 100, size=len(codes[::7])).astype(ctype)   # as unsigned numbers: above 255
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    clay, cwords = encode_column(adac, gpu_ctx, codes, counts)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    kmax = int(keys.max())
    assert (mc.code_numbers(codes) == 255).any() and (mc.code_numbers(codes) < 255).any()
    for base, span in ((1, kmax), (1000, 50001), (kmax - 10, 11), (kmax + 5, 100)):   # all, a part, the end, none
        exp, inside = check_build(gpu_ctx, keys, codes, klay, kwords, clay, cwords, counts, base, span, fill,
                                  what=(base, span))
        assert inside.any() == (base <= kmax) and (not inside.all() or base == 1)
        assert (exp[span:] == fill).all()   # the pad
        exp_m, inside_m = check_build(gpu_ctx, keys, codes, klay, kwords, clay, cwords, counts, base, span, fill, keep,
                                      d_mask, (base, span, "masked"))
        assert inside_m.sum() < inside.sum() or not inside.any()
    # the staged reader (keys at w > 32), duplicate keys with agreeing codes, and with disagreeing ones
    counts2 = np.array([3000, 257], dtype=np.uint32)
    k2 = (np.uint64(1 << 40) + rng.integers(0, 900, size=int(counts2.sum())).astype(np.uint64))
    k2[0], k2[1] = 0, (1 << 41)
    agree = (k2 % np.uint64(251)).astype(ctype)
    klay2, kwords2 = encode_column(adac, gpu_ctx, k2, counts2)
    alay, awords = encode_column(adac, gpu_ctx, agree, counts2)
    assert mc.mapped_forms(klay2, 1 << 40, 1000, alay)[0] == "staged-slice"
    exp, inside = check_build(gpu_ctx, k2, agree, klay2, kwords2, alay, awords, counts2, 1 << 40, 1000, fill, what="agree")
    assert inside.sum() == len(k2) - 2 and len(mc.built_map(k2, agree, 1 << 40, 1000, fill)[2]) == 0
    c2 = codes[:len(k2)]
    clay2, cwords2 = encode_column(adac, gpu_ctx, c2, counts2)
    assert len(mc.built_map(k2, c2, 1 << 40, 1000, fill)[2]) > 100
    check_build(gpu_ctx, k2, c2, klay2, kwords2, clay2, cwords2, counts2, 1 << 40, 1000, fill, what="disagree")


# ---------------------------------------------------------------------------------------------------------------------
# 13. Q5-shaped: a map built from an orders-like table under a bitmap, a lineitem-like table grouped through it
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_q5_round_trip(adac, gpu_ctx):
    rng = np.random.default_rng(74)
    n_orders, nations = 50_000, 25
    o_orderkey = sparse_keys(n_orders).astype(np.int32)
    o_nation = rng.integers(0, nations, size=n_orders).astype(np.uint8)   # the nation of the order's customer
    o_orderdate = rng.integers(8000, 10600, size=n_orders).astype(np.int32)
    per = rng.integers(1, 8, size=n_orders)
    l_orderkey = np.repeat(o_orderkey, per)
    n_items = len(l_orderkey)
    l_price = rng.integers(90000, 10500000, size=n_items).astype(np.int64)
    oc, lc = segments_of(n_orders), segments_of(n_items)
    okey, onat = encode_column(adac, gpu_ctx, o_orderkey, oc), encode_column(adac, gpu_ctx, o_nation, oc)
    odate = encode_column(adac, gpu_ctx, o_orderdate, oc)
    lkey, price = encode_column(adac, gpu_ctx, l_orderkey, lc), encode_column(adac, gpu_ctx, l_price, lc)
    # WHERE o_orderdate >= 8766 AND o_orderdate < 9131, as a bitmap over the orders
    ow = (n_orders + 63) // 64
    d_obm, d_ocnt = gpu_ctx.alloc(ow * 8), gpu_ctx.alloc(len(oc) * 8)
    odate[0].scan_select_between(odate[1], 8766, 9130, d_obm, d_ocnt)
    year = (o_orderdate >= 8766) & (o_orderdate <= 9130)
    assert 0.05 < year.mean() < 0.5
    base, span = 1, int(o_orderkey.max())
    d_map = gpu_ctx.alloc(mc.map_bytes(span) + 8)
    d_map.upload(np.full(mc.map_bytes(span) // 8 + 1, POISON, dtype=np.uint64))
    d_rows = gpu_ctx.alloc(len(oc) * 8)
    okey[0].scan_build_map(okey[1], onat[0], onat[1], base, span, d_map, 255, d_rows, d_obm)
    exp_map = np.full(mc.map_bytes(span), 255, dtype=np.uint8)
    exp_map[(o_orderkey[year] - base).astype(np.int64)] = o_nation[year]
    got_map = d_map.download(np.uint8, mc.map_bytes(span) + 8)
    assert np.array_equal(got_map[:-8], exp_map) and (got_map[-8:] == 0xFF).all()
    assert int(d_rows.download(np.uint64, len(oc)).sum()) == int(year.sum())
    d_s, d_c, d_r = gpu_ctx.alloc((nations + 1) * 8), gpu_ctx.alloc((nations + 1) * 8), gpu_ctx.alloc(len(lc) * 8)
    lkey[0].scan_group_sum_mapped(lkey[1], price[0], price[1], d_map, base, span, nations, d_s, d_c, d_r)
    code = exp_map[(l_orderkey - base).astype(np.int64)].astype(np.int64)
    g = np.minimum(code, nations)
    exp_s, exp_c = np.zeros(nations + 1, dtype=np.uint64), np.zeros(nations + 1, dtype=np.uint64)
    np.add.at(exp_s, g, l_price.astype(np.uint64))
    np.add.at(exp_c, g, np.uint64(1))
    s, c = d_s.download(np.uint64, nations + 1), d_c.download(np.uint64, nations + 1)
    assert np.array_equal(s, exp_s) and np.array_equal(c, exp_c)
    assert int(c[nations]) > int(c[:nations].sum()) > 0   # most rows are dropped by the filter, some are not
    assert int(d_r.download(np.uint64, len(lc)).sum()) == n_items
