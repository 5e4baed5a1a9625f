"""adac_bp_scan_sum_product: SUM(a * b) per segment over two columns of DuckDB BITPACKING blocks walked in step,
under an optional selection bitmap.  Blocks from the oracle's compress, expected values from numpy (uint64 products
after widening each factor by its own signedness) over the oracle's scan of the same blocks; outputs pre-filled with
0xA5 plus a guard word; every call made twice (tests/bp_pair_cases.py)."""
import numpy as np
import pytest

from oracle import bitpacking as bp
from bp_pair_cases import ALL, GROUP, GUARD, Dev, Packed, check_sum_product, four_masks, fresh, kind_column, untouched

pytestmark = pytest.mark.gpu
DELTA, FOR = bp.MODE_DELTA_FOR, bp.MODE_FOR


def pair(adac, ctx, va, vb, mode_a=bp.MODE_AUTO, mode_b=bp.MODE_AUTO, **kw):
    return Dev(adac, ctx, Packed(va, mode_a, **kw)), Dev(adac, ctx, Packed(vb, mode_b, **kw))


# 1 -----------------------------------------------------------------------------------------------------------------
def every_pair_columns(dtype_a, dtype_b, seed):
    rng = np.random.default_rng(seed)
    a = kind_column(dtype_a, rng, [g % 5 for g in range(25)])
    b = kind_column(dtype_b, rng, [(g // 5) % 5 for g in range(25)])
    return a, b, rng


def test_every_pair_of_modes_under_every_mask(adac, gpu_ctx):
    va, vb, rng = every_pair_columns(np.int32, np.int32, 1)
    da, db = pair(adac, gpu_ctx, va, vb)
    a, b = da.p, db.p
    assert len(a.modes) == 26 and len(b.modes) == 26
    seen = {(ma, mb) for (ma, _), (mb, _) in zip(a.modes, b.modes)}
    assert seen >= {(x, y) for x in (1, 2, 3, 4) for y in (1, 2, 3, 4)}, sorted(seen)
    masks = four_masks(a.span, rng)
    # the steps mask has clear and full steps inside groups where exactly one column is DELTA_FOR (width >= 1)
    one_delta = [g for g, ((ma, wa), (mb, wb)) in enumerate(zip(a.modes, b.modes))
                 if ((ma == DELTA and wa > 0) != (mb == DELTA and wb > 0))]
    assert len(one_delta) >= 6
    group_steps = [masks["steps"][g * GROUP:(g + 1) * GROUP:64] for g in one_delta]
    assert all(not st.all() for st in group_steps)                       # clear steps inside every such group
    assert all(st[np.argmin(st):].any() for st in group_steps)           # and a full one after the first clear one
    want = check_sum_product(da, db)
    assert want[0] != 0
    for name, m in masks.items():
        w = check_sum_product(da, db, m)
        assert w == {"zero": [0], "one": want}.get(name, w)
    # the roles swapped: the same products
    assert check_sum_product(db, da, masks["random"]) == check_sum_product(da, db, masks["random"])


def test_width_zero_for_and_delta_for(adac, gpu_ctx):
    """Forced FOR over constant groups and forced DELTA_FOR over arithmetic progressions: the width-0 forms."""
    rng = np.random.default_rng(2)
    const = np.repeat(np.arange(100, 106, dtype=np.int64), GROUP)[:5 * GROUP + 777].astype(np.int32)
    ramp = (50 + 3 * np.arange(5 * GROUP + 777, dtype=np.int64)).astype(np.int32)
    noise = rng.integers(-1000, 1000, size=5 * GROUP + 777).astype(np.int16)
    pc, pr, pn = Packed(const, FOR), Packed(ramp, DELTA), Packed(noise)
    assert all(m == (FOR, 0) for m in pc.modes), pc.modes
    assert all(m == DELTA for m, _ in pr.modes) and any(w == 0 for _, w in pr.modes), pr.modes
    dc, dr, dn = (Dev(adac, gpu_ctx, p) for p in (pc, pr, pn))
    masks = four_masks(pc.span, rng)
    for x, y in ((dc, dr), (dr, dc), (dc, dn), (dn, dr), (dr, dr), (dc, dc)):
        check_sum_product(x, y)
        check_sum_product(x, y, masks["random"])
        check_sum_product(x, y, masks["steps"])


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("role", ["a", "b"])
def test_types(adac, gpu_ctx, dtype, role):
    dtype = np.dtype(dtype)
    vx, vy, rng = every_pair_columns(dtype, np.int32, 10 + dtype.itemsize + (dtype.kind == "i"))
    dx, dy = pair(adac, gpu_ctx, vx, vy)
    da, db = (dx, dy) if role == "a" else (dy, dx)
    check_sum_product(da, db)
    check_sum_product(da, db, rng.random(da.p.span) < 0.5)


def wide64(rng, mode, signed):
    n = 4 * GROUP + 777
    if mode == FOR:
        v = (1 << 40) + rng.integers(0, 1 << 36, size=n, dtype=np.uint64).astype(object)
        if signed:
            v = v - (1 << 41)
    else:
        lo, hi = (-(1 << 34), 1 << 34) if signed else (0, 1 << 35)
        v = (1 << 50) + np.cumsum(rng.integers(lo, hi, size=n).astype(object))
    return np.array(v, dtype=np.int64 if signed else np.uint64)


@pytest.mark.parametrize("mode", [FOR, DELTA])
def test_uint64_times_int64_wider_than_32_bits(adac, gpu_ctx, mode):
    rng = np.random.default_rng(20 + mode)
    da, db = pair(adac, gpu_ctx, wide64(rng, mode, False), wide64(rng, mode, True), mode, mode)
    for p in (da.p, db.p):
        assert all(m == mode and w > 32 for m, w in p.modes[:-1]), p.modes
    masks = four_masks(da.p.span, rng)
    check_sum_product(da, db)
    check_sum_product(da, db, masks["random"])
    check_sum_product(da, db, masks["steps"])
    check_sum_product(db, da, masks["steps"])


# 3 -----------------------------------------------------------------------------------------------------------------
def width_values(rng, w, mode, dtype, groups=3):
    """Groups of 2048 rows whose FOR fields / DELTA_FOR deltas span exactly w bits."""
    n = groups * GROUP + 777
    f = rng.integers(0, 1 << w, size=n, dtype=np.uint64)
    f[3::GROUP], f[9::GROUP] = 0, (1 << w) - 1
    if mode == FOR:
        return (f + np.uint64(1000)).astype(dtype)
    return np.array(1000 + np.cumsum(f.astype(object)), dtype=dtype)


@pytest.mark.parametrize("mode", [FOR, DELTA])
@pytest.mark.parametrize("wa,ta,wb,tb", [(21, np.uint64, 40, np.uint64), (17, np.uint32, 16, np.uint32),
                                         (21, np.int64, 40, np.int64)])
def test_stage_pieces_that_differ(adac, gpu_ctx, mode, wa, ta, wb, tb):
    rng = np.random.default_rng(30 + wa + mode)
    if mode == DELTA and np.dtype(ta).itemsize == 4:
        ta = tb = np.uint64   # 2048 deltas of 17 bits leave 32 bits
    da, db = pair(adac, gpu_ctx, width_values(rng, wa, mode, ta), width_values(rng, wb, mode, tb), mode, mode)
    assert all(m == (mode, wa) for m in da.p.modes[:-1]), da.p.modes
    assert all(m == (mode, wb) for m in db.p.modes[:-1]), db.p.modes
    masks = four_masks(da.p.span, rng)
    for x, y in ((da, db), (db, da)):
        check_sum_product(x, y)
        for name in ("random", "steps", "zero"):
            check_sum_product(x, y, masks[name])
    # a window of a few steps far into the group: whole pieces of both columns are passed over (FOR)
    far = np.zeros(da.p.span, dtype=bool)
    far[1990:2048] = far[GROUP + 1600:GROUP + 1700] = far[2 * GROUP + 64:2 * GROUP + 65] = True
    check_sum_product(da, db, far)


# 4 -----------------------------------------------------------------------------------------------------------------
def test_segmentation_that_differs(adac, gpu_ctx):
    rng = np.random.default_rng(40)
    n = 40 * GROUP + 777
    wide = rng.integers(0, 1 << 62, size=n, dtype=np.uint64)
    narrow = rng.integers(0, 200, size=n).astype(np.uint8)
    dw, dn = pair(adac, gpu_ctx, wide, narrow)
    assert dw.p.nseg == 3 and dn.p.nseg == 1 and dw.p.nseg != dn.p.nseg
    mask = rng.random(n) < 0.5
    for x, y in ((dw, dn), (dn, dw)):
        want = check_sum_product(x, y)
        assert len(want) == x.p.nseg
        check_sum_product(x, y, mask)
    adac.set_tuning("num_cus", 1)   # runs of groups that cross a's segment boundaries inside one wave
    try:
        check_sum_product(dw, dn, mask)
    finally:
        adac.set_tuning("num_cus", 0)


# 5 -----------------------------------------------------------------------------------------------------------------
def test_element_space_with_gaps(adac, gpu_ctx):
    rng = np.random.default_rng(50)
    counts = [3 * GROUP, 2 * GROUP + 777]
    out_offs = [37, 37 + counts[0] + 100]
    n = sum(counts)
    va = rng.integers(-(1 << 20), 1 << 20, size=n).astype(np.int32)
    vb = rng.integers(0, 1 << 10, size=n).astype(np.uint16)
    da, db = pair(adac, gpu_ctx, va, vb, counts=counts, out_offs=out_offs)
    a = da.p
    assert a.span == out_offs[1] + counts[1] and not a.cover[:37].any() and not a.cover[37 + counts[0]:out_offs[1]].any()
    mask = rng.random(a.nwords * 64) < 0.5
    want = check_sum_product(da, db, mask)
    noisy = mask.copy()                       # every bit no segment covers set: in the gaps and past the span
    noisy[:a.span][~a.cover] = True
    noisy[a.span:] = True
    assert check_sum_product(da, db, noisy) == want
    quiet = mask.copy()
    quiet[:a.span][~a.cover] = False
    quiet[a.span:] = False
    assert check_sum_product(da, db, quiet) == want
    check_sum_product(da, db)


# 6 -----------------------------------------------------------------------------------------------------------------
def test_same_column_twice_zero_rows_and_one_row(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(60)
    va, _, _ = every_pair_columns(np.int16, np.int16, 61)
    da = Dev(adac, ctx, Packed(va))
    want = check_sum_product(da, da)                       # a == b: the sum of squares
    assert want == [int((va.astype(np.int64) ** 2).sum())]
    check_sum_product(da, da, rng.random(da.p.span) < 0.5)
    # layouts without rows: d_sums is still written
    for counts in ([0, 0], [0]):
        dz = Dev(adac, ctx, Packed(np.zeros(0, np.int32), counts=counts))
        assert check_sum_product(dz, dz) == [0] * len(counts)
        for _ in range(2):
            d_sums = fresh(ctx, len(counts))
            dz.lay.scan_sum_product(None, dz.lay, None, d_sums)
            assert [int(x) for x in d_sums.download(np.uint64, len(counts))] == [0] * len(counts)
        d_sums = fresh(ctx, len(counts))   # without rows the blocks pointers are not looked at, aligned or not
        dz.lay.scan_sum_product(dz.d_blocks.ptr + 8, dz.lay, dz.d_blocks.ptr + 8, d_sums)
        assert [int(x) for x in d_sums.download(np.uint64, len(counts) + 1)] == [0] * len(counts) + [GUARD]
    empty = adac.BitpackingLayout(ctx, np.int32, np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    d_any = fresh(ctx, 4)
    empty.scan_sum_product(None, empty, None, d_any)
    empty.scan_sum_product(None, empty, None, None)
    assert untouched(d_any, 4)
    # a single 1-row column
    d1, d2 = pair(adac, ctx, np.array([-7], dtype=np.int8), np.array([1 << 63], dtype=np.uint64))
    assert check_sum_product(d1, d2) == [(-7 * (1 << 63)) & ((1 << 64) - 1)]
    check_sum_product(d2, d1, np.array([True]))
    assert check_sum_product(d1, d2, np.array([False])) == [0]


# 7 -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_accepted_segmentations(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(70)
    v = rng.integers(-5000, 5000, size=4873).astype(np.int32)
    u = rng.integers(0, 60000, size=4873).astype(np.uint16)
    one = Dev(adac, ctx, Packed(v, counts=[4873]))
    split = Dev(adac, ctx, Packed(u, counts=[3000, 1873]))          # the same rows, different groups
    short = Dev(adac, ctx, Packed(u[:2048], counts=[2048]))         # a different group count
    ctx2 = adac.Context(0)
    try:
        other = Dev(adac, ctx2, Packed(u, counts=[4873]))           # the same groups on another context
        same = Dev(adac, ctx, Packed(u, counts=[4873]))
        d_sums = fresh(ctx, 4)

        def rejected(call):
            with pytest.raises(adac.AdacError) as err:
                call()
            assert err.value.status == 1
            assert untouched(d_sums, 4)      # nothing was enqueued

        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, split.lay, split.d_blocks, d_sums))
        rejected(lambda: split.lay.scan_sum_product(split.d_blocks, one.lay, one.d_blocks, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, short.lay, short.d_blocks, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, other.lay, other.d_blocks, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks.ptr + 8, same.lay, same.d_blocks, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, same.lay, same.d_blocks.ptr + 8, d_sums))
        rejected(lambda: one.lay.scan_sum_product(None, same.lay, same.d_blocks, d_sums))
        twin = ctx.upload(one.p.buf)   # one layout object binds one buffer at a time: twice with two buffers is refused
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, one.lay, twin, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, same.lay, None, d_sums))
        rejected(lambda: one.lay.scan_sum_product(one.d_blocks, same.lay, same.d_blocks, None))
        assert adac.lib().adac_bp_scan_sum_product(None, one.d_blocks.ptr, same.lay._h, same.d_blocks.ptr, None,
                                                   d_sums.ptr) == 1
        assert adac.lib().adac_bp_scan_sum_product(one.lay._h, one.d_blocks.ptr, None, same.d_blocks.ptr, None,
                                                   d_sums.ptr) == 1
        assert untouched(d_sums, 4)
        check_sum_product(one, same)
    finally:
        ctx2.close()
    # different segments, the same groups: accepted and correct, per segment of the first layout
    x = Dev(adac, ctx, Packed(v, counts=[4096, 777]))
    y = Dev(adac, ctx, Packed(u, counts=[2048, 2825]))
    mask = rng.random(4873) < 0.5
    assert len(check_sum_product(x, y, mask)) == 2
    assert len(check_sum_product(y, x, mask)) == 2
    check_sum_product(x, y)
