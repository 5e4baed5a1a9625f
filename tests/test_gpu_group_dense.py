"""adac_scan_group_sum_dense / adac_scan_group_count_dense: SUM(value), COUNT(*) GROUP BY a dense integer key of any
cardinality on the packed bytes of both columns.  Expected values are numpy over the ORIGINAL columns
(dense_cases.expected: scan_member_cases.member_index for the index, np.add.at on uint64 for sums and counts mod 2^64).
Every call is made twice into poisoned outputs with one spare word after each, which must stay poison, and the two
results must be equal (dense_cases.run_sum / run_count)."""
import numpy as np
import pytest

import dense_cases as dc
import scan_member_cases as sm
from dense_cases import ALL_FORMS, DENSE_WINDOW, check_dense, dense_forms, expected, run_count, run_sum
from scan_member_cases import POISON
from scan_compare_cases import typed_column, COUNTS_TYPES, place_bits
from test_gpu_scan_select_compare import COUNTS4, gapped_offsets, half_mask
from test_gpu_sum_product import COUNTS3, encode_column, kind_columns, offsets_of, widen

gpu = pytest.mark.gpu
INVALID_ARGUMENT = 1


class Knob:
    def __init__(self, adac, name, value, default):
        self.adac, self.name, self.value, self.default = adac, name, value, default

    def __enter__(self):
        self.adac.set_tuning(self.name, self.value)

    def __exit__(self, *exc):
        self.adac.set_tuning(self.name, self.default)


def domain_around(vals, span):
    """(base pattern, span): a domain of up to `span` keys centred on the column's median, kept inside the type"""
    tb = 8 * vals.dtype.itemsize
    span = min(span, 1 << tb)
    mid = int(np.sort(sm.biased(vals))[len(vals) // 2])
    dlo = min(max(mid - span // 2, 0), (1 << tb) - span)
    return dlo ^ sm.sign_bit(vals.dtype), span


# ---------------------------------------------------------------------------------------------------------------------
# 1. every key width, each segment with a domain of its own inside its interval
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", sm.GRID_TYPES, ids=lambda t: np.dtype(t).name)
def test_key_width_grid(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    keys, vals, doms = dc.key_width_grid(dtype)
    nseg = 8 * dtype.itemsize
    counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    assert [int(w) for w in klay.get_descs()["width"]] == list(range(1, nseg + 1))
    assert len(set(int(w) for w in vlay.get_descs()["width"])) == 16
    rng = np.random.default_rng(41)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span))
    seen = set()
    for s, (base, span) in enumerate(doms):
        f = dense_forms(klay, base, span, vlay)
        assert f[s] not in (None, "header")
        seen |= set(f) | set(dense_forms(klay, base, span))
        _, _, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, what=(s + 1,))
        mine = inside[s * sm.ROWS_GRID:(s + 1) * sm.ROWS_GRID]
        assert mine.any() and (s == 0 or not mine.all()), s + 1   # rows inside and outside the domain
        check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, keep, d_mask, (s + 1, "masked"),
                    every_entry=False)
    # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 indices: no staged reader with direct adds)
    assert seen >= ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. every value width of the 8-byte types against a key at w = 13; sums that wrap, negative values
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("vtype", [np.uint64, np.int64], ids=lambda t: np.dtype(t).name)
def test_value_widths(adac, gpu_ctx, vtype):
    vtype = np.dtype(vtype)
    rng = np.random.default_rng(42 + vtype.itemsize + (vtype.kind == "i"))
    rows, nseg = 257, 64
    counts = np.full(nseg, rows, dtype=np.uint32)
    hot = 1000 + rng.integers(200, 4000, size=48)   # few distinct keys: many rows per sum
    keys = rng.choice(hot, size=rows * nseg).astype(np.uint32)
    keys[rng.random(rows * nseg) < 0.2] = 1000 + 7000   # outside the domains below
    keys[0::rows], keys[1::rows] = 1000, 1000 + (1 << 13) - 1
    vals = np.concatenate([sm.segment_at_width(rng, vtype, rows, w) for w in range(1, 65)])
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    assert all(int(w) == 13 for w in klay.get_descs()["width"])
    assert [int(w) for w in vlay.get_descs()["width"]] == list(range(1, 65))
    for base, span, acc in ((1000 + 200, DENSE_WINDOW, "window"), (1100, 5000, "direct")):
        f = dense_forms(klay, base, span, vlay)
        assert f == ["walk-" + acc] * 32 + ["staged-" + acc] * 32, f   # widths above 32 fall to the staged reader
        s, c, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, what=(acc,))
        assert inside.sum() > 200
    exact = {}
    for k, v in zip(keys[inside], vals[inside]):
        exact[int(k)] = exact.get(int(k), 0) + int(v)
    if vtype.kind == "u":
        assert any(x >= 2 ** 64 for x in exact.values()), "no sum wrapped"
    else:
        assert (vals[inside] < 0).any() and (vals[inside] > 0).any()
    assert all(int(s[k - base]) == x % 2 ** 64 for k, x in exact.items())


# ---------------------------------------------------------------------------------------------------------------------
# 3. every type pair: domains at the key type's ends, across zero, one key, 2^24 keys
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("vtype", dc.VALUE_TYPES, ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("ktype", sm.TYPES, ids=lambda t: np.dtype(t).name)
def test_every_type_pair(adac, gpu_ctx, ktype, vtype):
    keys, vals = typed_column(ktype), typed_column(vtype, side=1)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS_TYPES)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, COUNTS_TYPES)
    rng = np.random.default_rng(43)
    keep, d_mask = half_mask(gpu_ctx, rng, COUNTS_TYPES, None, int(klay.value_span))
    rows = 0
    for name, base, span in sm.typed_domains(ktype):
        big = span > 1 << 20
        _, c, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS_TYPES, base, span,
                                   what=(name,), every_entry=not big)
        if span == 1:
            assert inside.any(), name   # the type's minimum / maximum / -1 are rows of segment 0
        rows += int(inside.sum())
        if not big:
            check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS_TYPES, base, span, keep, d_mask,
                        (name, "masked"), every_entry=False)
    assert rows > 100


# ---------------------------------------------------------------------------------------------------------------------
# 4. segment shapes on either side: raw, ADAC_NO_MIN, padded, the recompact rule, wrapping frames, the all-ones min,
#    segments of 0 rows and 1 row, gaps, other offsets for the values
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_segment_shapes_on_either_side(adac, gpu_ctx):
    rng = np.random.default_rng(44)
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
            met |= set(dense_forms(lay, base, span, pv[0]))
            _, _, inside = check_dense(gpu_ctx, col, plain_v, lay, words, pv[0], pv[1], COUNTS3, base, span,
                                       what=(name, "keys", want))
            assert inside.any(), (name, want)
        base, span = 70000 - 5, 290   # the column as the values
        met |= set(dense_forms(pk[0], base, span, lay))
        check_dense(gpu_ctx, plain_k, col, pk[0], pk[1], lay, words, COUNTS3, base, span, what=(name, "values"),
                    every_entry=False)
    assert {"staged-direct", "staged-window", "walk-window", "walk-direct"} <= met, met
    # segments of 0 rows and 1 row, gaps between the key segments, the values at other offsets
    nn = int(COUNTS4.sum())
    keys = (rng.integers(0, 1 << 11, size=nn) + 5000).astype(np.int32)
    vals = rng.integers(0, 1 << 20, size=nn).astype(np.uint32)
    koffs = gapped_offsets(COUNTS4)
    voffs = np.array(offsets_of(COUNTS4, None), dtype=np.uint64) + np.uint64(13)
    klay, kwords = encode_column(adac, gpu_ctx, keys, COUNTS4, koffs)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, COUNTS4, voffs)
    f = dense_forms(klay, 5000 + 100, 1500, vlay)
    assert f[4] is None and f[8] is None and int(COUNTS4[0]) == 1
    _, _, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS4, 5000 + 100, 1500, what="gaps")
    assert inside.any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. several scan groups per segment: 24 577 rows is one row past a scan group; entries hit from both groups
# ---------------------------------------------------------------------------------------------------------------------
def two_group_column(dtype, w, span, want, seed=45):
    rng = np.random.default_rng(seed + w)
    n, frame = 24577, 5
    keys = (rng.integers(0, 2 ** w, size=n, dtype=np.uint64) + np.uint64(frame)).astype(dtype)
    base = frame + 2 ** w + 10 if want == "header" else frame + 3
    if w > 16 and want != "header":   # few of 2^w keys would fall into the domain: plant some
        keys[2::3] = base + rng.integers(0, span, size=len(keys[2::3]), dtype=np.uint64)
    keys[0], keys[1] = frame, frame + 2 ** w - 1
    if want != "header":
        keys[n - 1] = keys[5] = base + span // 2   # the second group's only row adds to an entry of the first
    vals = rng.integers(0, 1 << 9, size=n).astype(np.uint16)
    return keys, vals, base


GROUP_CASES = [(np.uint32, 10, 400, "walk-window"), (np.uint32, 22, 1 << 21, "walk-direct"),
               (np.uint64, 40, 500, "staged-window"), (np.uint64, 40, 60000, "staged-direct"),
               (np.uint64, 12, 50, "header")]


@gpu
@pytest.mark.parametrize("dtype,w,span,want", GROUP_CASES, ids=[c[3] for c in GROUP_CASES])
def test_several_groups_per_segment(adac, gpu_ctx, dtype, w, span, want):
    keys, vals, base = two_group_column(dtype, w, span, want)
    counts, offs = np.array([len(keys)], dtype=np.uint32), np.array([37], dtype=np.uint64)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts, offs)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    assert dense_forms(klay, base, span, vlay) == [want]
    _, c, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, what=want)
    assert inside.any() == (want != "header")
    if want != "header":
        assert inside[-1] and int(c[span // 2]) >= 2
    rng = np.random.default_rng(46)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, offs, int(klay.value_span))
    check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, keep, d_mask, (want, "masked"))


# ---------------------------------------------------------------------------------------------------------------------
# 6. run combining: the knob never changes a result
# ---------------------------------------------------------------------------------------------------------------------
def run_columns():
    """name -> (keys, counts, base, span, keep or None)"""
    rng = np.random.default_rng(47)
    counts = np.array([24577, 4099, 257], dtype=np.uint32)
    n = int(counts.sum())
    out = {}
    runs = rng.integers(1, 41, size=n // 8)
    srt = np.repeat(np.arange(len(runs), dtype=np.uint32) * 3 + 1000, runs)[:n]
    assert len(srt) == n
    out["sorted, runs of 1 to 40"] = (srt, counts, 1000 + 50, int(srt.max()) - 1000 - 100, None)
    out["sorted, a small domain"] = (srt, counts, int(srt[20000]), DENSE_WINDOW - 3, None)
    one = np.full(24577, 4242, dtype=np.uint32)
    one[0], one[1] = 4000, 4000 + 1023   # (a constant column would pack at one bit and leave the walk)
    out["one key"] = (one, counts[:1], 4100, 500, None)
    out["one key, direct"] = (one, counts[:1], 3000, 5000, None)
    k = 7000
    pat = np.tile(np.array([k, 90000, k, k, k + 1, k, k + 1, k, k, k], dtype=np.uint32), 300)
    pat[0], pat[1] = 6000, 6000 + (1 << 17) - 1
    keep = np.ones(len(pat), dtype=bool)
    keep[7::10] = False   # k, masked, k
    out["interrupted runs"] = (pat, np.array([len(pat)], dtype=np.uint32), 6990, 40000, keep)
    out["interrupted runs, window"] = (pat, np.array([len(pat)], dtype=np.uint32), 6990, 40, keep)
    return out


@gpu
@pytest.mark.parametrize("name", sorted(run_columns()))
def test_run_combining(adac, gpu_ctx, name):
    keys, counts, base, span, keep = run_columns()[name]
    rng = np.random.default_rng(48)
    vals = rng.integers(-3000, -1000, size=len(keys)).astype(np.int32)   # negative, packed against a frame
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    vlay, vwords = encode_column(adac, gpu_ctx, vals, counts)
    f = dense_forms(klay, base, span, vlay)
    assert all(x.startswith("walk") or x == "header" for x in f), f
    assert any(x == ("walk-window" if "window" in name or "small" in name or name == "one key" else "walk-direct")
               for x in f), f
    d_mask = None
    if keep is not None:
        d_mask = gpu_ctx.upload(dc.full_mask(keep, counts, offsets_of(counts, None), int(klay.value_span)))
        _, inside = sm.member_index(keys, base, span)
        assert (~inside).any() and (~keep).any()
    got = []
    for knob in (1, 0):
        with Knob(adac, "group_dense_combine", knob, 1):
            check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, keep, d_mask, (name, knob))
            got.append(run_sum(gpu_ctx, klay, kwords, vlay, vwords, base, span, d_mask))
    for x, y in zip(*got):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the mask: the keys' element space, gaps and the tail set, the values elsewhere, a bitmap a select scan wrote
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ktype,w,span", [(np.int32, 12, 2500), (np.uint16, 3, 5), (np.uint64, 40, 2500)])
def test_mask_geometry(adac, gpu_ctx, ktype, w, span):
    rng = np.random.default_rng(49 + w)
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
    span_words = (int(klay.value_span) + 63) // 64
    base = 1000 + 1
    keep = rng.random(n) < 0.5
    d_mask = gpu_ctx.upload(dc.full_mask(keep, COUNTS4, [int(o) for o in koffs], int(klay.value_span)))
    _, _, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS4, base, span, keep, d_mask, "gaps")
    assert inside.any()
    # a bitmap that adac_scan_select_between wrote on a layout with the keys' offsets
    flay, fwords = encode_column(adac, gpu_ctx, vals, COUNTS4, koffs)
    d_bm, d_cnt = gpu_ctx.alloc(span_words * 8), gpu_ctx.alloc(len(COUNTS4) * 8)
    d_bm.upload(np.full(span_words, POISON, dtype=np.uint64))
    flay.scan_select_between(fwords, 10000, 40000, d_bm, d_cnt)
    sel = (vals >= 10000) & (vals <= 40000)
    _, _, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, COUNTS4, base, span, sel, d_bm, "select")
    assert inside.any() and not sel.all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the header form reads nothing: the packed words of its segments overwritten, the results stay
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_header_form_reads_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(50)
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
    base, span = 500, 10000
    f = dense_forms(klay, base, span, vlay)
    assert f == ["walk-direct", "header", "walk-direct", "header"], f
    before = run_sum(gpu_ctx, klay, kwords, vlay, vwords, base, span)
    before_c = run_count(gpu_ctx, klay, kwords, base, span)
    for lay, words in ((klay, kwords), (vlay, vwords)):
        d = lay.get_descs()
        arena = words.download(np.uint64, int(lay.max_arena_words))
        for s in (1, 3):
            o, nw = int(d["word_off"][s]), (int(d["count"][s]) * int(d["width"][s]) + 63) // 64
            arena[o:o + nw] = POISON
        words.upload(arena)
    after = run_sum(gpu_ctx, klay, kwords, vlay, vwords, base, span)
    after_c = run_count(gpu_ctx, klay, kwords, base, span)
    for x, y in list(zip(before, after)) + list(zip(before_c, after_c)):
        assert np.array_equal(x, y)
    assert int(after[2][1]) == 0 and int(after[2][3]) == 0 and int(after[2][0]) > 0
    exp_s, exp_c, _ = expected(keys, vals, base, span)
    assert np.array_equal(after[0], exp_s) and np.array_equal(after[1], exp_c)


# ---------------------------------------------------------------------------------------------------------------------
# 9. the outputs that may be left out, values == keys, and the refusals
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_values_are_the_keys(adac, gpu_ctx):
    rng = np.random.default_rng(51)
    counts = np.array([257, 9000], dtype=np.uint32)
    keys = (rng.integers(0, 700, size=int(counts.sum())) + 300).astype(np.uint16)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts)
    base, span = 310, 600
    s, c, _ = check_dense(gpu_ctx, keys, keys, klay, kwords, klay, kwords, counts, base, span, what="values == keys")
    assert np.array_equal(s, c * (np.arange(span, dtype=np.uint64) + np.uint64(base)))   # t-weighted sums
    assert int(c.sum()) > 5000


@gpu
def test_argument_errors_write_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(52)
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
    span = 100
    d_s, d_c, d_r = gpu_ctx.alloc(span * 8), gpu_ctx.alloc(span * 8), gpu_ctx.alloc(2 * 8)
    d_mask = gpu_ctx.upload(np.full(nwords, POISON, dtype=np.uint64))
    bufs = ((d_s, span), (d_c, span), (d_r, 2), (d_mask, nwords))
    for b, nw in bufs[:3]:
        b.upload(np.full(nw, POISON, dtype=np.uint64))
    sm_, cn_ = klay.scan_group_sum_dense, klay.scan_group_count_dense
    i32max = 0x7FFFFFFF
    refused = [
        # key_span outside 1 ... 2^32, a domain that leaves the type
        lambda: sm_(kwords, vlay, vwords, 0, 0, d_s, d_c, d_r), lambda: cn_(kwords, 0, 0, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, 1 << 31, (1 << 32) + 1, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, i32max, 2, d_s, d_c, d_r), lambda: cn_(kwords, i32max - 9, 11, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords, 1 << 32, 10, d_s, d_c, d_r), lambda: cn_(kwords, 1 << 40, 10, d_c, d_r),
        lambda: small.scan_group_count_dense(kwords, 65530, 7, d_c, d_r),
        # a required output that is NULL; NULL words; words not 16-byte aligned
        lambda: sm_(kwords, vlay, vwords, 0, span, None, d_c, d_r), lambda: cn_(kwords, 0, span, None, d_r),
        lambda: sm_(None, vlay, vwords, 0, span, d_s, d_c, d_r), lambda: sm_(kwords, vlay, None, 0, span, d_s, d_c, d_r),
        lambda: cn_(None, 0, span, d_c, d_r),
        lambda: sm_(kwords.ptr + 8, vlay, vwords, 0, span, d_s, d_c, d_r),
        lambda: sm_(kwords, vlay, vwords.ptr + 8, 0, span, d_s, d_c, d_r), lambda: cn_(kwords.ptr + 8, 0, span, d_c, d_r),
        # per-segment counts that differ, layouts on different contexts
        lambda: sm_(kwords, other[0], other[1], 0, span, d_s, d_c, d_r),
        lambda: sm_(kwords, far, vwords, 0, span, d_s, d_c, d_r),
        # any two of the outputs and the mask overlapping
        lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_s, d_r), lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_c, d_s),
        lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_s.ptr + 8 * (span - 1), d_r),
        lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_c, d_c.ptr + 8 * (span - 1)),
        lambda: sm_(kwords, vlay, vwords, 0, span, d_mask, d_c, d_r, d_mask),
        lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_mask, d_r, d_mask),
        lambda: sm_(kwords, vlay, vwords, 0, span, d_s, d_c, d_mask.ptr + 8 * (nwords - 1), d_mask),
        lambda: cn_(kwords, 0, span, d_c, d_c), lambda: cn_(kwords, 0, span, d_mask, d_r, d_mask),
        lambda: cn_(kwords, 0, span, d_c, d_mask, d_mask),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(adac.AdacError) as e:
            call()
        assert e.value.status == INVALID_ARGUMENT, i
    with pytest.raises(Exception):
        klay.scan_group_sum_dense(kwords, None, vwords, 0, span, d_s, d_c, d_r)   # a NULL value layout
    assert adac.lib().adac_scan_group_sum_dense(klay._h, kwords.ptr, None, vwords.ptr, None, 0, span, d_s.ptr, d_c.ptr,
                                                d_r.ptr) == INVALID_ARGUMENT
    gpu_ctx.sync()
    for b, nw in bufs:
        assert (b.download(np.uint64, nw) == POISON).all()
    # a key layout without segments: ADAC_OK, and the outputs, whose size comes from key_span, are zero-filled
    e1, ev = adac.Layout(gpu_ctx, np.int32, np.zeros(0, np.uint32)), adac.Layout(gpu_ctx, np.uint16, np.zeros(0, np.uint32))
    e1.scan_group_sum_dense(None, ev, None, 1 << 31, span, d_s, d_c, None)
    assert not d_s.download(np.uint64, span).any() and not d_c.download(np.uint64, span).any()
    d_c.upload(np.full(span, POISON, dtype=np.uint64))
    e1.scan_group_count_dense(None, 1 << 31, span, d_c, None)
    assert not d_c.download(np.uint64, span).any()
    with pytest.raises(adac.AdacError):
        e1.scan_group_count_dense(None, (1 << 31) + 1, 1 << 32, d_c, None)
    # segments without rows only: everything written, nothing counted
    z1 = adac.Layout(gpu_ctx, np.int32, np.zeros(2, np.uint32))
    d_r.upload(np.full(2, POISON, dtype=np.uint64))
    z1.scan_group_count_dense(None, 0, span, d_c, d_r)
    assert d_r.download(np.uint64, 2).tolist() == [0, 0]
    # after the refusals the codec is still usable
    base, span2 = domain_around(keys, 1 << 16)
    _, _, inside = check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span2, what="afterwards")
    assert inside.any()
    far.close()
    ctx2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. Q18 at 200 000 lineitems: dense sum -> encode the sums -> select > threshold -> the bitmap as the member set of
#     a probe over o_orderkey
# ---------------------------------------------------------------------------------------------------------------------
def segments_of(n, rows=32767):
    return np.array([rows] * (n // rows) + ([n % rows] if n % rows else []), dtype=np.uint32)


@gpu
def test_q18_round_trip(adac, gpu_ctx):
    rng = np.random.default_rng(53)
    n_orders = 50_000
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)   # sparse-increasing, as dbgen's
    per = rng.integers(1, 8, size=n_orders)
    l_orderkey = np.repeat(o_orderkey, per)
    n_items = len(l_orderkey)
    assert 190_000 < n_items < 210_000
    l_quantity = rng.integers(1, 51, size=n_items).astype(np.int32)
    threshold = 180
    oc, lc = segments_of(n_orders), segments_of(n_items)
    okey = encode_column(adac, gpu_ctx, o_orderkey, oc)
    lkey, qty = encode_column(adac, gpu_ctx, l_orderkey, lc), encode_column(adac, gpu_ctx, l_quantity, lc)
    base, span = 1, int(o_orderkey.max())
    sc_ = segments_of(span)
    d_sums = gpu_ctx.alloc(span * 8)
    d_sums.upload(np.full(span, POISON, dtype=np.uint64))
    lkey[0].scan_group_sum_dense(lkey[1], qty[0], qty[1], base, span, d_sums)
    exp_sums = np.zeros(span, dtype=np.uint64)
    np.add.at(exp_sums, (l_orderkey - base).astype(np.int64), l_quantity.astype(np.uint64))
    assert np.array_equal(d_sums.download(np.uint64, span), exp_sums)
    slay = adac.Layout(gpu_ctx, np.uint64, sc_)
    d_swords = gpu_ctx.alloc(slay.max_arena_words * 8 + 16).zero()
    slay.encode(d_sums, d_swords)
    sw, ow = (span + 63) // 64, (n_orders + 63) // 64
    d_set, d_scnt = gpu_ctx.alloc(sw * 8), gpu_ctx.alloc(len(sc_) * 8)
    d_obm, d_ocnt = gpu_ctx.alloc(ow * 8), gpu_ctx.alloc(len(oc) * 8)
    for buf, nw in ((d_set, sw), (d_obm, ow)):
        buf.upload(np.full(nw, POISON, dtype=np.uint64))
    slay.scan_select_between(d_swords, threshold + 1, POISON, d_set, d_scnt)
    okey[0].scan_select_member(okey[1], d_set, base, span, d_obm, d_ocnt)
    large = exp_sums[(o_orderkey - base).astype(np.int64)] > threshold
    assert 0.02 < large.mean() < 0.9   # some orders qualify and some do not
    assert int(d_scnt.download(np.uint64, len(sc_)).sum()) == int(large.sum())
    assert np.array_equal(d_obm.download(np.uint64, ow), place_bits(large, oc, offsets_of(oc, None), n_orders))
    assert int(d_ocnt.download(np.uint64, len(oc)).sum()) == int(large.sum())
