"""adac_scan_select_member / adac_scan_count_member / adac_scan_build_member: test a row's value against a bit set
indexed by value, and build such a set from the wanted rows of a packed column.  Expected values are numpy over the
ORIGINAL columns (scan_member_cases.member_mask / built_set, held against Python integers in
test_scan_member_forms.py).  Every call is made twice into poisoned outputs (0xFF bytes in d_counts, d_bitmap, d_set and
one spare word after each, which must stay untouched), and the count form is held against the select's counts
(scan_member_cases.run_member / run_build).  Every probe set carries ones in the tail bits of its last word."""
import importlib

import numpy as np
import pytest

import scan_member_cases as sm
from scan_member_cases import POISON, check_build, check_member, kind, random_set, run_build, run_member
from scan_compare_cases import typed_column, COUNTS_TYPES, place_bits
from test_gpu_scan_select_compare import COUNTS4, gapped_offsets, half_mask
from test_gpu_sum_product import COUNTS3, encode_column, kind_columns, offsets_of

gpu = pytest.mark.gpu
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")
INVALID_ARGUMENT = 1


def device_forms(lay, base, bits):
    return forms.member_form_groups(lay.get_descs(), kind(lay.dtype), base, bits)


def both_ways(ctx, vals, lay, words, counts, base, bits, set_words, rng, val_offs=None, what=""):
    """probe and build, without and with a 50 % mask"""
    check_member(ctx, vals, lay, words, counts, base, bits, set_words, val_offs=val_offs, what=(what, "no mask"))
    check_build(ctx, vals, lay, words, counts, base, bits, what=(what, "build"))
    keep, d_mask = half_mask(ctx, rng, counts, val_offs, int(lay.value_span))
    check_member(ctx, vals, lay, words, counts, base, bits, set_words, keep, d_mask, val_offs, what=(what, "masked"))
    check_build(ctx, vals, lay, words, counts, base, bits, keep, d_mask, what=(what, "masked build"))
    d_mask.free()


def domain_around(vals, bits):
    """(base pattern, bits): a domain of up to `bits` bits centred on the column's median, kept inside the type"""
    tb = 8 * vals.dtype.itemsize
    bits = min(bits, 1 << tb)
    mid = int(np.sort(sm.biased(vals))[len(vals) // 2])
    dlo = min(max(mid - bits // 2, 0), (1 << tb) - bits)
    return dlo ^ sm.sign_bit(vals.dtype), bits


# ---------------------------------------------------------------------------------------------------------------------
# 1. every width, each segment with a domain of its own inside its interval
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", sm.GRID_TYPES, ids=lambda t: np.dtype(t).name)
def test_width_grid(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    vals, doms = sm.width_grid(dtype)
    nseg = 8 * dtype.itemsize
    counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
    lay, words = encode_column(adac, gpu_ctx, vals, counts)
    assert [int(w) for w in lay.get_descs()["width"]] == list(range(1, nseg + 1))
    rng = np.random.default_rng(21)
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(lay.value_span))
    seen = set()
    for s, (base, bits, set_words) in enumerate(doms):
        got = sm.classes_of(vals[s * sm.ROWS_GRID:(s + 1) * sm.ROWS_GRID], base, bits, set_words)
        assert got["set"] and got["clear"] and (s == 0 or (got["below"] and got["above"])), (s + 1, got)
        f = device_forms(lay, base, bits)
        assert f[s] != "header"
        seen |= set(f)
        check_member(gpu_ctx, vals, lay, words, counts, base, bits, set_words, what=(s + 1, "no mask"))
        check_member(gpu_ctx, vals, lay, words, counts, base, bits, set_words, keep, d_mask, what=(s + 1, "masked"))
        check_build(gpu_ctx, vals, lay, words, counts, base, bits, what=(s + 1, "build"))
        check_build(gpu_ctx, vals, lay, words, counts, base, bits, keep, d_mask, what=(s + 1, "masked build"))
    assert {"header", "walk-slice", "walk-direct", "staged-slice"} <= seen, seen


# ---------------------------------------------------------------------------------------------------------------------
# 2. every type: domains at the type's ends, across zero, one bit, 2^24 bits
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", sm.TYPES, ids=lambda t: np.dtype(t).name)
def test_every_type(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    vals = typed_column(dtype)
    lay, words = encode_column(adac, gpu_ctx, vals, COUNTS_TYPES)
    rng = np.random.default_rng(22)
    selected = 0
    for name, base, bits in sm.typed_domains(dtype):
        set_words = random_set(rng, bits)
        if bits == 1:
            set_words[0] |= np.uint64(1)
        hit = check_member(gpu_ctx, vals, lay, words, COUNTS_TYPES, base, bits, set_words, what=(dtype.name, name))
        if bits == 1:
            assert hit.any(), name   # the type's minimum / maximum / -1 are rows of segment 0
        selected += int(hit.sum())
        keep, d_mask = half_mask(gpu_ctx, rng, COUNTS_TYPES, None, int(lay.value_span))
        check_member(gpu_ctx, vals, lay, words, COUNTS_TYPES, base, bits, set_words, keep, d_mask, what=(name, "masked"))
        check_build(gpu_ctx, vals, lay, words, COUNTS_TYPES, base, bits, keep, d_mask, what=(name, "masked build"))
        d_mask.free()
        built = check_build(gpu_ctx, vals, lay, words, COUNTS_TYPES, base, bits, what=(dtype.name, name, "build"))
        # the set a build wrote, probed: exactly the rows of the domain
        _, inside = sm.member_index(vals, base, bits)
        again = check_member(gpu_ctx, vals, lay, words, COUNTS_TYPES, base, bits, built, what=(name, "built set"))
        assert np.array_equal(again, inside)
    assert selected > 100


# ---------------------------------------------------------------------------------------------------------------------
# 3. segment shapes: raw, ADAC_NO_MIN, padded, the recompact rule, wrapping frames
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_segment_shapes(adac, gpu_ctx):
    rng = np.random.default_rng(23)
    met = set()
    for name, (vals, rule, pad, check) in kind_columns().items():
        lay, words = encode_column(adac, gpu_ctx, vals, COUNTS3, rule=rule, pad=pad)
        assert check(lay.get_descs()), (name, lay.get_descs())
        for want_bits in (64, 1 << 17):
            base, bits = domain_around(vals, want_bits)
            met |= set(device_forms(lay, base, bits))
            set_words = random_set(rng, bits)
            mid = np.sort(sm.biased(vals))[len(vals) // 2]   # the median is a member, whatever else is
            sm.set_bit(set_words, int(mid) - (base ^ sm.sign_bit(vals.dtype)), True)
            hit = sm.member_mask(vals, base, bits, set_words)
            assert hit.any(), (name, want_bits)
            both_ways(gpu_ctx, vals, lay, words, COUNTS3, base, bits, set_words, rng, what=(name, want_bits))
    assert {"staged-direct", "staged-slice", "walk-slice"} <= met, met


# ---------------------------------------------------------------------------------------------------------------------
# 4. the window of the set in on-chip memory
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_slice_geometry(adac, gpu_ctx):
    rng = np.random.default_rng(24)
    counts = np.array([3000, 5000], dtype=np.uint32)
    f0, f1 = 1000, 50000
    s0 = (rng.integers(0, 1 << 12, size=3000) + f0).astype(np.uint32)
    s1 = (rng.integers(0, 1 << 20, size=5000) + f1).astype(np.uint32)
    s0[0], s0[-1], s1[0], s1[-1] = f0, f0 + (1 << 12) - 1, f1, f1 + (1 << 20) - 1
    s0[5] = f0 + 77
    s1[1:2000] = f1 + rng.integers(0, 70000, size=1999)   # rows for the windows at the interval's start
    vals = np.concatenate([s0, s1])
    lay, words = encode_column(adac, gpu_ctx, vals, counts)
    assert [int(w) for w in lay.get_descs()["width"]] == [12, 20]
    cases = []
    for k in (0, 1, 31):   # (frame - set_base) mod 32: the phase of the window's first bit
        cases.append(("phase %d" % k, f0 - 96 - k, 96 + k + 1001, ["walk-slice", "header"]))
        cases.append(("phase %d to the end of the type's interval" % k, f0 - 32 - k, 6000, ["walk-slice", "header"]))
    cases += [("inside the interval", f0 + 500, 1001, ["walk-slice", "header"]),
              ("one bit", f0 + 77, 1, ["walk-slice", "header"]),
              ("span 65536", f1 + 100, 65536, ["header", "walk-slice"]),
              ("span 65537", f1 + 100, 65537, ["header", "walk-direct"]),
              ("span 65536 from bit 31: the largest window", f1 - 31, 31 + 65536, ["header", "walk-slice"]),
              ("span 65537 from bit 31", f1 - 31, 31 + 65537, ["header", "walk-direct"]),
              ("both segments", 0, (1 << 21) - 5, ["walk-slice", "walk-direct"])]
    for name, base, bits, want in cases:
        assert device_forms(lay, base, bits) == want, name
        assert bits % 64 or name == "span 65536"
        set_words = random_set(rng, bits)   # every tail bit of the last word set
        if bits == 1:
            set_words[0] |= np.uint64(1)
        hit = sm.member_mask(vals, base, bits, set_words)
        assert hit.any(), name
        both_ways(gpu_ctx, vals, lay, words, counts, base, bits, set_words, rng, what=name)
    # tail bits alone select nothing: an empty set whose last word is all ones past set_bits
    for name, base, bits, _ in cases:
        if bits % 64:
            empty = random_set(rng, bits, 0.0)
            assert int(empty[-1]) != 0
            bm, cn = run_member(gpu_ctx, lay, words, gpu_ctx.upload(empty), base, bits)
            assert not bm.any() and cn == [0, 0], name


# ---------------------------------------------------------------------------------------------------------------------
# 5. bitmap geometry
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gapped", [False, True], ids=["back to back", "gaps"])
@pytest.mark.parametrize("dtype,w,reader", [(np.int32, 13, "walk"), (np.uint16, 3, "staged")])
def test_bitmap_geometry(adac, gpu_ctx, gapped, dtype, w, reader):
    rng = np.random.default_rng(25 + w)
    val_offs = gapped_offsets(COUNTS4) if gapped else None
    n = int(COUNTS4.sum())
    vals = (rng.integers(0, 2 ** w, size=n) + 1000).astype(dtype)
    lay, words = encode_column(adac, gpu_ctx, vals, COUNTS4, val_offs)
    base, bits = 1000 + 2 ** w // 4, 2 ** w // 2
    f = device_forms(lay, base, bits)
    assert f[4] is None and f[8] is None
    assert any(x is not None and x.startswith(reader) for x in f), f
    set_words = random_set(rng, bits)
    both_ways(gpu_ctx, vals, lay, words, COUNTS4, base, bits, set_words, rng, val_offs, what=reader)
    _, cn = run_member(gpu_ctx, lay, words, gpu_ctx.upload(set_words), base, bits)
    assert cn[4] == 0 and cn[8] == 0  # segments without rows


# ---------------------------------------------------------------------------------------------------------------------
# 6. segments longer than one scan group: neighbouring groups share bitmap words and add into one count
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype,n,w,bits,want", [(np.uint32, 24577, 10, 600, "walk-slice"),
                                                 (np.uint32, 24577, 22, 1 << 21, "walk-direct"),
                                                 (np.uint32, 24577, 3, 5, "staged-slice"),
                                                 (np.uint8, 65537, 6, 40, "walk-slice"),
                                                 (np.uint8, 65537, 2, 3, "staged-slice"),
                                                 (np.uint64, 24577, 14, 9000, "walk-slice"),
                                                 (np.uint64, 24577, 40, 1 << 24, "staged-direct"),
                                                 (np.uint64, 24577, 40, 60000, "staged-slice"),
                                                 (np.uint64, 24577, 12, 50, "header")])
def test_several_groups_per_segment(adac, gpu_ctx, dtype, n, w, bits, want):
    rng = np.random.default_rng(26 + w)
    frame = 5
    vals = (rng.integers(0, 2 ** w, size=n, dtype=np.uint64) + np.uint64(frame)).astype(dtype)
    vals[0], vals[n - 1] = frame, frame + 2 ** w - 1
    counts, offs = np.array([n], dtype=np.uint32), np.array([37], dtype=np.uint64)
    lay, words = encode_column(adac, gpu_ctx, vals, counts, offs)
    base = frame + 2 ** w + 10 if want == "header" else frame + 1
    if bits >= 60000 and w == 40:   # few of 2^40 values would fall into the domain: plant some
        vals2 = vals.copy()
        vals2[1:n - 1:3] = base + rng.integers(0, bits, size=len(vals2[1:n - 1:3]), dtype=np.uint64)
        vals = vals2
        lay, words = encode_column(adac, gpu_ctx, vals, counts, offs)
    assert device_forms(lay, base, bits) == [want]
    set_words = random_set(rng, bits)
    hit = sm.member_mask(vals, base, bits, set_words)
    assert hit.any() == (want != "header")
    both_ways(gpu_ctx, vals, lay, words, counts, base, bits, set_words, rng, offs, what=want)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the build
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_build(adac, gpu_ctx):
    rng = np.random.default_rng(27)
    # every row the same value
    counts = np.array([9000, 700], dtype=np.uint32)
    same = np.full(9700, 4242, dtype=np.int32)
    lay, words = encode_column(adac, gpu_ctx, same, counts)
    st, cn = run_build(gpu_ctx, lay, words, 4000, 1000)
    exp = np.zeros(sm.set_words_for(1000), dtype=np.uint64)
    exp[242 >> 6] = np.uint64(1 << (242 & 63))
    assert np.array_equal(st, exp) and cn == [9000, 700]
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, 9700)
    check_build(gpu_ctx, same, lay, words, counts, 4000, 1000, keep, d_mask, what="duplicates, masked")
    # every row outside the domain: decided by the descriptor, and decided row by row
    vals = np.concatenate([rng.integers(0, 11, size=4850), rng.integers(4000, 4096, size=4850)]).astype(np.uint32) + 100
    rng.shuffle(vals)
    vals[0], vals[-1] = 100, 100 + 4095
    lay, words = encode_column(adac, gpu_ctx, vals, counts)
    for base, bits, want in ((100 + 4096, 333, "header"), (100 + 200, 333, "walk-slice")):
        assert device_forms(lay, base, bits) == [want, want]
        st, cn = run_build(gpu_ctx, lay, words, base, bits)
        assert not st.any() and cn == [0, 0], want
    # two segments that write the same set words, one through the window and one with global atomics
    a = (rng.integers(0, 1 << 10, size=9000) + 1000).astype(np.uint32)
    b = rng.integers(0, 1 << 20, size=700).astype(np.uint32)
    b[:400] = 1000 + rng.integers(0, 1 << 10, size=400)
    a[0], a[-1], b[-2], b[-1] = 1000, 1000 + 1023, 0, (1 << 20) - 1
    vals = np.concatenate([a, b])
    lay, words = encode_column(adac, gpu_ctx, vals, counts)
    assert device_forms(lay, 0, 1 << 18) == ["walk-slice", "walk-direct"]
    exp = check_build(gpu_ctx, vals, lay, words, counts, 0, 1 << 18, what="slice and direct")
    only_a, _ = sm.built_set(a, 0, 1 << 18)
    only_b, _ = sm.built_set(b, 0, 1 << 18)
    assert (only_a & only_b).any() and (only_a & ~only_b).any() and (only_b & ~only_a).any()   # shared words, both add
    assert np.array_equal(exp, only_a | only_b)
    check_build(gpu_ctx, vals, lay, words, counts, 0, (1 << 18) - 13, keep, d_mask, what="slice and direct, masked")


# ---------------------------------------------------------------------------------------------------------------------
# 8. Q4's shape: compare -> build -> probe -> grouped count
# ---------------------------------------------------------------------------------------------------------------------
def segments_of(n, rows=32767):
    return np.array([rows] * (n // rows) + ([n % rows] if n % rows else []), dtype=np.uint32)


@gpu
def test_q4_round_trip(adac, gpu_ctx):
    rng = np.random.default_rng(28)
    n_orders = 20_000
    idx = np.arange(n_orders, dtype=np.int64)
    o_orderkey = ((idx // 8) * 32 + idx % 8 + 1).astype(np.int32)   # sparse-increasing, as dbgen's
    o_priority = rng.integers(0, 5, size=n_orders).astype(np.uint8)
    per = rng.integers(1, 8, size=n_orders)
    l_orderkey = np.repeat(o_orderkey, per)
    n_items = len(l_orderkey)
    assert 70_000 < n_items < 90_000
    ship = rng.integers(8036, 10562, size=n_items).astype(np.int32)
    l_commit = (ship + rng.integers(-30, 60, size=n_items)).astype(np.int32)
    l_receipt = (ship + rng.integers(-60, 31, size=n_items)).astype(np.int32)
    oc, lc = segments_of(n_orders), segments_of(n_items)
    assert len(lc) == 3
    okey, prio = encode_column(adac, gpu_ctx, o_orderkey, oc), encode_column(adac, gpu_ctx, o_priority, oc)
    lkey, commit, receipt = (encode_column(adac, gpu_ctx, v, lc) for v in (l_orderkey, l_commit, l_receipt))
    base, bits = 1, int(o_orderkey.max())
    late = l_commit < l_receipt
    member = np.isin(o_orderkey, l_orderkey[late])
    assert 0.2 < member.mean() < 0.9
    lw, ow, sw = (n_items + 63) // 64, (n_orders + 63) // 64, sm.set_words_for(bits)
    d_lbm, d_obm, d_set = gpu_ctx.alloc(lw * 8), gpu_ctx.alloc(ow * 8), gpu_ctx.alloc(sw * 8)
    d_lcnt, d_ocnt = gpu_ctx.alloc(len(lc) * 8), gpu_ctx.alloc(len(oc) * 8)
    d_sums, d_gcnt = gpu_ctx.alloc(6 * 8), gpu_ctx.alloc(6 * 8)
    for buf, nw in ((d_lbm, lw), (d_obm, ow), (d_set, sw)):
        buf.upload(np.full(nw, POISON, dtype=np.uint64))
    commit[0].scan_select_compare(commit[1], receipt[0], receipt[1], adac.CMP_LT, d_lbm, d_lcnt)
    lkey[0].scan_build_member(lkey[1], base, bits, d_set, d_lcnt, d_lbm)
    assert int(d_lcnt.download(np.uint64, len(lc)).sum()) == int(late.sum())
    okey[0].scan_select_member(okey[1], d_set, base, bits, d_obm, d_ocnt)
    okey[0].scan_group_sum_valid(okey[1], prio[0], prio[1], d_obm, 5, d_sums, d_gcnt)
    assert np.array_equal(d_obm.download(np.uint64, ow), place_bits(member, oc, offsets_of(oc, None), n_orders))
    assert int(d_ocnt.download(np.uint64, len(oc)).sum()) == int(member.sum())
    exp = np.bincount(o_priority[member], minlength=5)
    assert [int(x) for x in d_gcnt.download(np.uint64, 6)] == [int(x) for x in exp] + [0]


# ---------------------------------------------------------------------------------------------------------------------
# 9. Q12's IN list: a 7-valued code against a set of two
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_q12_in_list(adac, gpu_ctx):
    rng = np.random.default_rng(29)
    n = 70_001
    mode = rng.integers(0, 7, size=n).astype(np.uint8)
    counts = segments_of(n)
    lay, words = encode_column(adac, gpu_ctx, mode, counts)
    assert all(int(w) == 3 for w in lay.get_descs()["width"])
    assert device_forms(lay, 0, 7) == ["staged-slice"] * len(counts)
    in_list = np.array([POISON & ~0x7F | (1 << 2) | (1 << 5)], dtype=np.uint64)   # 'MAIL', 'SHIP'; the tail set
    hit = check_member(gpu_ctx, mode, lay, words, counts, 0, 7, in_list)
    assert np.array_equal(hit, np.isin(mode, [2, 5]))
    keep, d_mask = half_mask(gpu_ctx, rng, counts, None, n)
    check_member(gpu_ctx, mode, lay, words, counts, 0, 7, in_list, keep, d_mask, what="masked")
    # a domain of the two codes' span alone, and the codes as a domain that does not start at the frame
    check_member(gpu_ctx, mode, lay, words, counts, 2, 4, np.array([POISON & ~0xF | 0b1001], dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals, all decided on the host before anything is enqueued
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_argument_errors_write_nothing(adac, gpu_ctx):
    rng = np.random.default_rng(30)
    counts = np.array([100, 3000], dtype=np.uint32)
    vals = np.concatenate([sm.segment_at_width(rng, np.int32, int(c), 17) for c in counts])
    lay, words = encode_column(adac, gpu_ctx, vals, counts)
    small = adac.Layout(gpu_ctx, np.uint16, counts)
    nwords = (int(lay.value_span) + 63) // 64
    d_bm, d_cnt, d_set = gpu_ctx.alloc(nwords * 8), gpu_ctx.alloc(16), gpu_ctx.alloc(nwords * 8)
    d_mask = gpu_ctx.upload(np.full(nwords, POISON, dtype=np.uint64))
    for buf in (d_bm, d_set):
        buf.upload(np.full(nwords, POISON, dtype=np.uint64))
    d_cnt.upload(np.full(2, POISON, dtype=np.uint64))
    sel, cnt, bld = lay.scan_select_member, lay.scan_count_member, lay.scan_build_member
    i32max = 0x7FFFFFFF
    refused = [
        # set_bits outside 1 ... 2^32
        lambda: sel(words, d_set, 0, 0, d_bm, d_cnt), lambda: cnt(words, d_set, 0, 0, d_cnt),
        lambda: bld(words, 0, 0, d_set, d_cnt),
        lambda: sel(words, d_set, 1 << 31, (1 << 32) + 1, d_bm, d_cnt),
        lambda: bld(words, 1 << 31, (1 << 32) + 1, d_set, d_cnt),
        # a domain that leaves the type: past int32's maximum, from -1 across the pattern space, bits above the type
        lambda: sel(words, d_set, i32max, 2, d_bm, d_cnt), lambda: cnt(words, d_set, i32max - 9, 11, d_cnt),
        lambda: bld(words, i32max, 2, d_set, d_cnt),
        lambda: sel(words, d_set, (1 << 31) + 1, 1 << 32, d_bm, d_cnt),
        lambda: sel(words, d_set, 1 << 32, 10, d_bm, d_cnt), lambda: bld(words, 1 << 40, 10, d_set, d_cnt),
        lambda: small.scan_count_member(words, d_set, 65530, 7, d_cnt),
        lambda: small.scan_build_member(words, 0, (1 << 16) + 1, d_set, d_cnt),
        # NULL counts, set, words; words not 16-byte aligned
        lambda: sel(words, d_set, 0, 100, d_bm, None), lambda: cnt(words, d_set, 0, 100, None),
        lambda: bld(words, 0, 100, d_set, None),
        lambda: sel(words, None, 0, 100, d_bm, d_cnt), lambda: cnt(words, None, 0, 100, d_cnt),
        lambda: bld(words, 0, 100, None, d_cnt),
        lambda: sel(None, d_set, 0, 100, d_bm, d_cnt), lambda: bld(None, 0, 100, d_set, d_cnt),
        lambda: sel(words.ptr + 8, d_set, 0, 100, d_bm, d_cnt), lambda: cnt(words.ptr + 8, d_set, 0, 100, d_cnt),
        lambda: bld(words.ptr + 8, 0, 100, d_set, d_cnt),
        # the bitmap: NULL, the mask itself
        lambda: sel(words, d_set, 0, 100, None, d_cnt), lambda: sel(words, d_set, 0, 100, d_mask, d_cnt, d_mask),
        # the set aliasing the bitmap or the mask
        lambda: sel(words, d_bm, 0, 100, d_bm, d_cnt), lambda: sel(words, d_mask, 0, 100, d_bm, d_cnt, d_mask),
        lambda: cnt(words, d_mask, 0, 100, d_cnt, d_mask), lambda: bld(words, 0, 100, d_mask, d_cnt, d_mask),
        lambda: bld(words, 0, 100, d_mask.ptr + 8, d_cnt, d_mask),
    ]
    for i, call in enumerate(refused):
        with pytest.raises(adac.AdacError) as e:
            call()
        assert e.value.status == INVALID_ARGUMENT, i
    gpu_ctx.sync()
    for buf in (d_bm, d_set, d_mask):
        assert (buf.download(np.uint64, nwords) == POISON).all()
    assert (d_cnt.download(np.uint64, 2) == POISON).all()
    # the largest domains are legal: the whole of int32 (only the argument check: 512 MiB of set are not allocated),
    # decided here by a layout without segments, which returns before the device is touched
    e1 = adac.Layout(gpu_ctx, np.int32, np.zeros(0, np.uint32))
    e1.scan_select_member(None, d_set, 1 << 31, 1 << 32, None, None)
    e1.scan_count_member(None, d_set, 1 << 31, 1 << 32, None)
    e1.scan_build_member(None, 1 << 31, 1 << 32, d_set, None)
    with pytest.raises(adac.AdacError):
        e1.scan_count_member(None, d_set, (1 << 31) + 1, 1 << 32, None)
    assert (d_set.download(np.uint64, nwords) == POISON).all()
    # segments without rows only: the counts are written, the built set is empty
    z1 = adac.Layout(gpu_ctx, np.int32, np.zeros(2, np.uint32))
    z1.scan_select_member(None, d_set, 0, 100, None, d_cnt)
    assert d_cnt.download(np.uint64, 2).tolist() == [0, 0]
    d_cnt.upload(np.full(2, POISON, dtype=np.uint64))
    z1.scan_build_member(None, 0, 100, d_set, d_cnt)
    assert d_cnt.download(np.uint64, 2).tolist() == [0, 0]
    assert d_set.download(np.uint64, nwords)[:2].tolist() == [0, 0] and int(d_set.download(np.uint64, nwords)[2]) == POISON
    base, bits = domain_around(vals, 1 << 16)
    both_ways(gpu_ctx, vals, lay, words, counts, base, bits, random_set(rng, bits), rng, what="after the refusals")
