"""adac_bp_scan_select_compare / adac_bp_scan_count_compare: the rows where value(a) <cmp> value(b) for two columns of
DuckDB BITPACKING blocks walked in step, as a selection bitmap in a's element space and as counts per segment of a,
nothing decoded to HBM.  Expected values: numpy over the oracle's scan of the same blocks, the raw values compared as
Python integers (tests/bp_compare_cases.py).  Conventions of tests/bp_pair_cases.py: every output pre-filled with 0xA5
plus a guard word, every call made twice, the bitmap compared word for word over all of its words.

1 every pair of cursor kinds under every comparison and mask, five pairs of types;  2 bit phases at which neighbouring
segments and groups share bitmap words;  3 groups answered from the two headers (payload overwritten with 0xFF);
4 segment ends that differ;  5 one layout twice, and a Q12-shaped chain;  6 grids of 1 and 3 CUs;  7 argument errors.
A case takes well under a second of device time on an MI355X; the Python-integer reference dominates."""
import numpy as np
import pytest

from bp_compare_cases import (ALL_CMPS, DELTA, EQ, FOR, GT, LINEAR, LT, check_select_compare, cursor_kinds,
                              for_payloads, relation)
from bp_pair_cases import GROUP, GUARD, Dev, Packed, four_masks, fresh, kind_column, pack_bits, untouched
from oracle import bitpacking as bp

pytestmark = pytest.mark.gpu

TYPE_PAIRS = [(np.int32, np.int32), (np.uint8, np.uint64), (np.int16, np.uint32), (np.int64, np.uint64),
              (np.int8, np.int8)]
KINDS_A = [0, 1, 2, 3, 4] * 5
KINDS_B = [k for k in range(5) for _ in range(5)]


# 1 -----------------------------------------------------------------------------------------------------------------
def every_kind_columns(ta, tb, seed):
    """a's kind cycles with the group, b's with the group divided by five: 25 groups + a 777-row tail.  A third of the
    rows of b's FOR groups (kinds 3 and 4) and of its tail take a's value where b's type holds it, so EQ has hits
    inside walked groups; rows of b's constant, arithmetic and sorted groups are left alone, since one foreign value
    turns such a group into FOR and the nine kind pairs asserted below would be lost.  A uint64 b gets values >= 2^63
    in its wide FOR groups."""
    rng = np.random.default_rng(seed)
    a = kind_column(ta, rng, KINDS_A)
    b = kind_column(tb, rng, KINDS_B)
    n = len(a)
    info = np.iinfo(b.dtype)
    g = np.arange(n) // GROUP
    in_for = (g >= 15)                                   # b's groups 15 .. 24 (kinds 3, 4) and the tail
    if b.dtype == np.uint64:
        top = in_for & (g >= 20) & (g < 25) & (rng.random(n) < 0.25)
        b[top] = np.uint64(1 << 63) + rng.integers(0, 1 << 62, size=int(top.sum()), dtype=np.uint64)
    ai = a.astype(object)
    fits = np.asarray((ai >= int(info.min)) & (ai <= int(info.max)), dtype=bool)
    if b.dtype.kind == "i":     # the codec refuses a signed group whose max - min leaves the type
        starts = np.arange(0, n, GROUP)
        sizes = np.diff(np.append(starts, n))
        lo = np.repeat(np.minimum.reduceat(b, starts), sizes).astype(object)
        hi = np.repeat(np.maximum.reduceat(b, starts), sizes).astype(object)
        mid, reach = (lo + hi) // 2, int(info.max) // 2 - 1     # any two values this near the middle are storable
        fits &= np.asarray((ai >= mid - reach) & (ai <= mid + reach), dtype=bool)
    take = in_for & fits & (rng.random(n) < 1 / 3)
    b[take] = a[take].astype(b.dtype)
    return a, b


@pytest.fixture(scope="module")
def kind_cases(adac, gpu_ctx):
    """The five type pairs of case 1 on the device, with their relation: built once, read by cases 1 and 6."""
    out = {}
    for i, (ta, tb) in enumerate(TYPE_PAIRS):
        a, b = every_kind_columns(ta, tb, 100 + i)
        da, db = Dev(adac, gpu_ctx, Packed(a)), Dev(adac, gpu_ctx, Packed(b))
        assert len(a) == 25 * GROUP + 777 == 51977
        out[(ta, tb)] = (da, db, relation(da.p, db.p), relation(db.p, da.p))
    return out


def test_cases_reach_every_kind_pair_and_wide_for_on_both_sides(kind_cases):
    pairs, wide_a, wide_b = set(), False, False
    for da, db, _, _ in kind_cases.values():
        pairs |= set(zip(cursor_kinds(da.p), cursor_kinds(db.p)))
        wide_a |= any(m == bp.MODE_FOR and w > 16 for m, w in da.p.modes)
        wide_b |= any(m == bp.MODE_FOR and w > 16 for m, w in db.p.modes)
    assert pairs == {(x, y) for x in (LINEAR, FOR, DELTA) for y in (LINEAR, FOR, DELTA)}, sorted(pairs)
    assert wide_a and wide_b
    da, db, _, _ = kind_cases[(np.int64, np.uint64)]
    assert (da.p.raw < 0).any() and (db.p.raw >= np.uint64(1 << 63)).any()


@pytest.mark.parametrize("ta,tb", TYPE_PAIRS, ids=lambda t: np.dtype(t).name)
def test_every_kind_pair_every_comparison(kind_cases, ta, tb):
    da, db, rel, rel_swapped = kind_cases[(ta, tb)]
    rng = np.random.default_rng(110)
    masks = four_masks(da.p.span, rng)
    hits = {}
    for name, mask in [("none", None)] + list(masks.items()):
        d_valid = None if mask is None else da.ctx.upload(pack_bits(mask, da.p.nwords))
        for cmp in ALL_CMPS:
            bits, counts, _ = check_select_compare(da, db, cmp, mask, d_valid, rel=rel)
            hits[(name, cmp)] = sum(counts)
    n = da.p.span
    assert hits[("none", LT)] + hits[("none", EQ)] + hits[("none", GT)] == n
    assert hits[("none", EQ)] > 1000 and hits[("none", LT)] > 0 and hits[("none", GT)] > 0
    assert all(hits[("zero", cmp)] == 0 for cmp in ALL_CMPS)
    # the other order: b's FOR groups, a third of them a's values, against every kind of a
    for mask in (None, masks["random"]):
        for cmp in ALL_CMPS:
            check_select_compare(db, da, cmp, mask, rel=rel_swapped, count_form=mask is None)


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [1, 63, 64, 65])
def test_bit_phase_and_shared_words(adac, gpu_ctx, phase):
    rng = np.random.default_rng(200 + phase)
    counts = [2053, 1, 0, 4096, 777]
    n = sum(counts)
    a = rng.integers(-3000, 3000, size=n).astype(np.int32)
    b = rng.integers(-3000, 3000, size=n).astype(np.int16)
    same = rng.random(n) < 1 / 3
    b[same] = a[same]
    b[2053] = a[2053] + 1                  # the one-row segment: a < b
    da = Dev(adac, gpu_ctx, Packed(a, counts=counts, phase=phase))
    db = Dev(adac, gpu_ctx, Packed(b, counts=counts, phase=phase))
    p = da.p
    assert p.span == phase + n and not p.cover[:phase].any()
    assert (p.group_start[1] % 64 != 0) == (phase % 64 != 0)     # off a word's edge, neighbours share bitmap words
    rel = relation(p, db.p)
    long_mask = rng.random((p.nwords + 3) * 64) < 0.5          # words past the span: they change nothing
    long_words = pack_bits(long_mask, p.nwords + 3)
    for cmp in ALL_CMPS:
        bits, cnt, _ = check_select_compare(da, db, cmp, rel=rel)
        assert not bits[:phase].any() and cnt[2] == 0 and cnt[1] == (1 if cmp & LT else 0)
        got = check_select_compare(da, db, cmp, long_mask, mask_words=long_words, rel=rel)
        short = check_select_compare(da, db, cmp, long_mask[:p.span], rel=rel, count_form=False)
        assert got[1] == short[1] and np.array_equal(got[0], short[0])
    ones = np.ones(p.nwords * 64, dtype=bool)                  # bits below the phase and past the span set
    le, gt = (check_select_compare(da, db, cmp, ones, rel=rel)[1] for cmp in (LT | EQ, GT))
    assert [x + y for x, y in zip(le, gt)] == counts


# 3 -----------------------------------------------------------------------------------------------------------------
def damaged(adac, ctx, p):
    """The column on the device a second time, the payload bytes of every FOR group overwritten with 0xFF."""
    d = Dev(adac, ctx, p)
    buf = p.buf.copy()
    spans = for_payloads(p)
    for off, nbytes in spans:
        buf[off:off + nbytes] = 0xFF
    d.d_blocks = ctx.upload(buf)
    return d, len(spans)


def test_header_answers_read_no_payload(adac, gpu_ctx):
    rng = np.random.default_rng(300)
    n = 3 * GROUP + 777
    mask = rng.random(n) < 0.5

    def both(a, b):
        pa, pb = Packed(a), Packed(b)
        return (Dev(adac, gpu_ctx, pa), Dev(adac, gpu_ctx, pb)), (damaged(adac, gpu_ctx, pa), damaged(adac, gpu_ctx, pb))

    # disjoint intervals in every group: a in [1000, 1000 + 2^10), b in [5000, 5000 + 2^11)
    a = (1000 + rng.integers(0, 1 << 10, size=n)).astype(np.int32)
    b = (5000 + rng.integers(0, 1 << 11, size=n)).astype(np.uint16)
    (da, db), ((xa, na), (xb, nb)) = both(a, b)
    assert all(m == bp.MODE_FOR and w >= 1 for m, w in da.p.modes + db.p.modes) and na == nb == 4
    for x, y, bx, by in ((da, db, xa, xb), (db, da, xb, xa)):
        rel = relation(x.p, y.p)
        for cmp in ALL_CMPS:
            for m in (None, mask):
                want = check_select_compare(x, y, cmp, m, rel=rel)
                got = check_select_compare(bx, by, cmp, m, rel=rel)       # the intact values' expectation
                assert got[1] == want[1] and np.array_equal(got[0], want[0])
                assert sum(want[1]) in (0, n if m is None else int(mask.sum()))
    # the damage is real: the decode of the damaged buffer differs
    d_out = gpu_ctx.alloc(n * 4)
    xa.lay.unpack(xa.d_blocks, d_out)
    assert not np.array_equal(d_out.download(np.int32, n), a)
    # two constant columns: one comparison per group
    ca, cb = np.full(n, -5, dtype=np.int8), np.full(n, 250, dtype=np.uint8)
    cb[GROUP:2 * GROUP] = 251
    dca, dcb = Dev(adac, gpu_ctx, Packed(ca)), Dev(adac, gpu_ctx, Packed(cb))
    assert all(m == bp.MODE_CONSTANT for m, _ in dca.p.modes + dcb.p.modes)
    for cmp in ALL_CMPS:
        for m in (None, mask):
            assert sum(check_select_compare(dca, dcb, cmp, m)[1]) == (0 if not cmp & LT else n if m is None
                                                                       else int(mask.sum()))
            check_select_compare(dcb, dca, cmp, m, count_form=False)
            check_select_compare(dcb, dcb, cmp, m, count_form=False)
    # overlapping intervals are walked: only the intact buffers are held against numpy
    b2 = (1500 + rng.integers(0, 1 << 11, size=n)).astype(np.uint16)
    b2[::7] = a[::7]
    db2 = Dev(adac, gpu_ctx, Packed(b2))
    assert all(m == bp.MODE_FOR for m, _ in db2.p.modes)
    rel = relation(da.p, db2.p)
    for cmp in ALL_CMPS:
        for m in (None, mask):
            bits, cnt, _ = check_select_compare(da, db2, cmp, m, rel=rel)
    assert 0 < sum(check_select_compare(da, db2, EQ, rel=rel, count_form=False)[1]) < n


# 4 -----------------------------------------------------------------------------------------------------------------
def test_segment_ends_that_differ(adac, gpu_ctx):
    rng = np.random.default_rng(400)
    n = int(2.3 * 262144 / 8) + 1234
    wide = rng.integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)
    narrow = rng.integers(0, 256, size=n).astype(np.uint8)
    wide[::5] = narrow[::5]
    dw, dn = Dev(adac, gpu_ctx, Packed(wide)), Dev(adac, gpu_ctx, Packed(narrow))
    assert dw.p.nseg == 3 and dn.p.nseg == 1
    mask = rng.random(n) < 0.5
    for x, y in ((dw, dn), (dn, dw)):
        rel = relation(x.p, y.p)
        for cmp in ALL_CMPS:
            _, counts, _ = check_select_compare(x, y, cmp, rel=rel)
            assert len(counts) == x.p.nseg                 # per segment of the first layout
            check_select_compare(x, y, cmp, mask, rel=rel, count_form=cmp == LT)
    assert sum(check_select_compare(dw, dn, EQ, count_form=False)[1]) >= (n + 4) // 5


# 5 -----------------------------------------------------------------------------------------------------------------
def test_same_layout_twice(adac, gpu_ctx):
    rng = np.random.default_rng(500)
    a, _ = every_kind_columns(np.int16, np.int16, 501)
    da = Dev(adac, gpu_ctx, Packed(a))
    mask = rng.random(len(a)) < 0.5
    for cmp in ALL_CMPS:
        assert sum(check_select_compare(da, da, cmp)[1]) == (len(a) if cmp & EQ else 0)
        assert sum(check_select_compare(da, da, cmp, mask)[1]) == (int(mask.sum()) if cmp & EQ else 0)


def test_q12_shaped_chain(adac, gpu_ctx):
    """receipt BETWEEN one year -> commit < receipt under it -> ship < commit under that -> SUM(ship) under the last"""
    ctx = gpu_ctx
    rng = np.random.default_rng(510)
    n = 5 * GROUP + 777
    ship, commit, receipt = (rng.integers(8036, 10562, size=n).astype(np.int32) for _ in range(3))
    ds, dc, dr = (Dev(adac, ctx, Packed(v)) for v in (ship, commit, receipt))
    p = dr.p
    lo, hi = 8766, 9130
    for _ in range(2):
        d_bm1, d_cnt1 = fresh(ctx, p.nwords), fresh(ctx, p.nseg)
        dr.lay.scan_select_between(dr.d_blocks, lo, hi, d_bm1, d_cnt1)
        sel1 = (receipt >= lo) & (receipt <= hi)
        assert np.array_equal(d_bm1.download(np.uint64, p.nwords), pack_bits(sel1, p.nwords)[:p.nwords])
        sel2, cnt2, d_bm2 = check_select_compare(dc, dr, LT, sel1, d_valid=d_bm1)
        assert np.array_equal(sel2, sel1 & (commit < receipt)) and cnt2 == [int(sel2.sum())]
        sel3, cnt3, d_bm3 = check_select_compare(ds, dc, LT, sel2, d_valid=d_bm2)
        assert np.array_equal(sel3, sel2 & (ship < commit)) and 0 < cnt3[0] < cnt2[0] < int(sel1.sum())
        d_sum = fresh(ctx, 1)
        ds.lay.scan_sum(ds.d_blocks, d_sum, d_bm3)
        got = d_sum.download(np.uint64, 2)
        assert int(got[0]) == int(ship[sel3].astype(np.int64).sum()) and int(got[1]) == GUARD


# 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cus", [1, 3])
def test_grid_sizes(adac, kind_cases, num_cus):
    """Few waves: each walks a run of many groups of every kind."""
    da, db, rel, _ = kind_cases[(np.int32, np.int32)]
    masks = four_masks(da.p.span, np.random.default_rng(600))
    adac.set_tuning("num_cus", num_cus)
    try:
        for cmp in ALL_CMPS:
            check_select_compare(da, db, cmp, rel=rel)
            check_select_compare(da, db, cmp, masks["random"], rel=rel)
        check_select_compare(da, db, LT | EQ, masks["steps"], rel=rel)
    finally:
        adac.set_tuning("num_cus", 0)


def test_grid_sizes_across_segments(adac, gpu_ctx):
    """One CU's waves over three segments of a: a wave's run of groups crosses segment ends."""
    rng = np.random.default_rng(610)
    counts = [9 * GROUP + 5, 3, 14 * GROUP + 100]
    n = sum(counts)
    a = rng.integers(-100, 100, size=n).astype(np.int32)
    b = rng.integers(-60, 60, size=n).astype(np.int8)          # (max - min has to fit the signed type)
    da, db = Dev(adac, gpu_ctx, Packed(a, counts=counts)), Dev(adac, gpu_ctx, Packed(b, counts=counts))
    rel = relation(da.p, db.p)
    mask = rng.random(n) < 0.5
    for num_cus in (1, 3):
        adac.set_tuning("num_cus", num_cus)
        try:
            for cmp in ALL_CMPS:
                check_select_compare(da, db, cmp, mask if cmp & 1 else None, rel=rel)
        finally:
            adac.set_tuning("num_cus", 0)


# 7 -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_layouts_without_rows(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(700)
    v = rng.integers(-5000, 5000, size=4873).astype(np.int32)
    u = rng.integers(0, 60000, size=4873).astype(np.uint16)
    one = Dev(adac, ctx, Packed(v, counts=[4873]))
    same = Dev(adac, ctx, Packed(u, counts=[4873]))
    short = Dev(adac, ctx, Packed(u[:2 * GROUP], counts=[2 * GROUP]))         # one group shorter
    nwords = one.p.nwords
    ctx2 = adac.Context(0)
    try:
        other = Dev(adac, ctx2, Packed(u, counts=[4873]))                   # the same groups on another context
        d_bitmap, d_counts = fresh(ctx, nwords), fresh(ctx, 1)

        def rejected(call):
            with pytest.raises(adac.AdacError) as err:
                call()
            assert err.value.status == 1
            assert untouched(d_bitmap, nwords) and untouched(d_counts, 1)   # nothing was enqueued

        sel = lambda x, xb, y, yb, cmp, bm, cnt, val=None: (      # noqa: E731
            lambda: x.lay.scan_select_compare(xb, y.lay, yb, cmp, bm, cnt, val))
        cnt = lambda x, xb, y, yb, cmp, c, val=None: (            # noqa: E731
            lambda: x.lay.scan_count_compare(xb, y.lay, yb, cmp, c, val))
        for cmp in (0, 7, 8, 1 << 31):
            rejected(sel(one, one.d_blocks, same, same.d_blocks, cmp, d_bitmap, d_counts))
            rejected(cnt(one, one.d_blocks, same, same.d_blocks, cmp, d_counts))
        rejected(sel(one, one.d_blocks, short, short.d_blocks, 1, d_bitmap, d_counts))
        rejected(cnt(short, short.d_blocks, one, one.d_blocks, 1, d_counts))
        rejected(sel(one, one.d_blocks, other, other.d_blocks, 1, d_bitmap, d_counts))
        rejected(cnt(one, one.d_blocks, other, other.d_blocks, 1, d_counts))
        rejected(sel(one, one.d_blocks, same, same.d_blocks, 1, d_bitmap, d_counts, d_bitmap))   # bitmap == validity
        rejected(sel(one, one.d_blocks, same, same.d_blocks, 1, None, d_counts))
        rejected(sel(one, one.d_blocks, same, same.d_blocks, 1, d_bitmap, None))
        rejected(cnt(one, one.d_blocks, same, same.d_blocks, 1, None))
        rejected(sel(one, one.d_blocks.ptr + 8, same, same.d_blocks, 1, d_bitmap, d_counts))
        rejected(sel(one, one.d_blocks, same, same.d_blocks.ptr + 8, 1, d_bitmap, d_counts))
        rejected(cnt(one, one.d_blocks.ptr + 8, same, same.d_blocks, 1, d_counts))
        rejected(sel(one, None, same, same.d_blocks, 1, d_bitmap, d_counts))
        twin = ctx.upload(one.p.buf)   # one layout object binds one buffer at a time: twice with two buffers is refused
        rejected(sel(one, one.d_blocks, one, twin, 2, d_bitmap, d_counts))
        rejected(cnt(one, one.d_blocks, one, twin, 2, d_counts))
        L = adac.lib()
        assert L.adac_bp_scan_select_compare(None, one.d_blocks.ptr, same.lay._h, same.d_blocks.ptr, None, 1,
                                             d_bitmap.ptr, d_counts.ptr) == 1
        assert L.adac_bp_scan_count_compare(one.lay._h, one.d_blocks.ptr, None, same.d_blocks.ptr, None, 1,
                                            d_counts.ptr) == 1
        assert untouched(d_bitmap, nwords) and untouched(d_counts, 1)
        check_select_compare(one, same, LT, rng.random(4873) < 0.5)        # and the accepted call is right
        check_select_compare(one, same, GT | EQ)
    finally:
        ctx2.close()
    # layouts without rows: OK, the counts are written (zero), no bitmap word exists
    for counts in ([0, 0], [0]):
        dz = Dev(adac, ctx, Packed(np.zeros(0, np.int32), counts=counts))
        assert check_select_compare(dz, dz, EQ)[1] == [0] * len(counts)
        d_bitmap, d_counts = fresh(ctx, 2), fresh(ctx, len(counts))
        dz.lay.scan_select_compare(None, dz.lay, None, LT, None, d_counts)    # span 0: NULL bitmap, NULL blocks
        assert [int(x) for x in d_counts.download(np.uint64, len(counts) + 1)] == [0] * len(counts) + [GUARD]
        d_counts = fresh(ctx, len(counts))
        dz.lay.scan_select_compare(dz.d_blocks.ptr + 8, dz.lay, dz.d_blocks.ptr + 8, GT, d_bitmap, d_counts)
        assert [int(x) for x in d_counts.download(np.uint64, len(counts) + 1)] == [0] * len(counts) + [GUARD]
        assert untouched(d_bitmap, 2)
    empty = adac.BitpackingLayout(ctx, np.int32, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    d_any = fresh(ctx, 4)
    empty.scan_select_compare(None, empty, None, LT, d_any, d_any)
    empty.scan_count_compare(None, empty, None, LT, None)
    empty.scan_select_compare(None, empty, None, LT, None, None)
    assert untouched(d_any, 4)
