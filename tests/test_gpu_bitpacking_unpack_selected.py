"""adac_bp_unpack_selected: the values (and element indices) of the rows a selection bitmap keeps, densely, straight
from DuckDB BITPACKING blocks.  Blocks from the oracle's compress, expected values from numpy over the oracle's scan
of the same blocks (tests/bp_pair_cases.py): per segment the decoded rows under the mask, concatenated.  Both outputs
hold total_values slots plus a guard word, every byte pre-filled with 0xA5; every call is made twice; every byte from
slot `total` on must still read 0xA5 afterwards."""
import numpy as np
import pytest

import bp_fuzz_columns as fz
from bp_pair_cases import ALL, GROUP, Dev, Packed, four_masks, fresh, kind_column, pack_bits, untouched
from oracle import bitpacking as bp
from test_gpu_bitpacking_sum_product import wide64, width_values

pytestmark = pytest.mark.gpu
DELTA, FOR = bp.MODE_DELTA_FOR, bp.MODE_FOR


def filled(ctx, nbytes):
    return ctx.alloc(nbytes).upload(np.full(nbytes, 0xA5, dtype=np.uint8))


def expected(p, mask):
    """(values, ids) of the rows of Packed `p` whose element is set in `mask` (bools over the element space; shorter
    than the span: the rest is clear), segment by segment."""
    m = np.zeros(max(p.span, len(mask)), dtype=bool)
    m[:len(mask)] = mask
    vals, ids = [np.zeros(0, p.dtype)], [np.zeros(0, np.uint64)]
    for o, s in zip(p.out_offs, p.segs):
        o = int(o)
        keep = m[o:o + len(s)]
        vals.append(s[keep])
        ids.append((o + np.flatnonzero(keep)).astype(np.uint64))
    return np.concatenate(vals), np.concatenate(ids)


def check_selected(dev, mask, ids=True, want_total=True):
    p, ctx = dev.p, dev.ctx
    want_v, want_i = expected(p, mask)
    total = len(want_v)
    n = int(p.counts.sum())
    assert dev.lay.total_values == n
    ts = p.dtype.itemsize
    d_mask = ctx.upload(pack_bits(mask, p.nwords))
    for _ in range(2):
        d_out, d_ids = filled(ctx, n * ts + 8), filled(ctx, n * 8 + 8)
        got_total = dev.lay.unpack_selected(dev.d_blocks, d_mask, d_out, d_ids if ids else None, want_total)
        if want_total:
            assert got_total == total
        else:
            assert got_total is None
            ctx.sync()
        raw = d_out.download(np.uint8, n * ts + 8)
        got_v = raw[:total * ts].view(p.dtype)
        bad = np.flatnonzero(got_v != want_v)
        assert len(bad) == 0, (bad[:8], got_v[bad[:8]], want_v[bad[:8]])
        assert np.all(raw[total * ts:] == 0xA5)          # nothing at or past slot `total`, the guard included
        raw = d_ids.download(np.uint8, n * 8 + 8)
        if ids:
            got_i = raw[:total * 8].view(np.uint64)
            bad = np.flatnonzero(got_i != want_i)
            assert len(bad) == 0, (bad[:8], got_i[bad[:8]], want_i[bad[:8]])
            assert np.all(raw[total * 8:] == 0xA5)
        else:
            assert np.all(raw == 0xA5)
    return total


def groups_of(p):
    """(first element, rows) of every metadata group"""
    for o, s in zip(p.out_offs, p.segs):
        for g in range((len(s) + GROUP - 1) // GROUP):
            yield int(o) + g * GROUP, min(GROUP, len(s) - g * GROUP)


def far_window(p):
    """a few steps far into each group, one lone row in the second step: whole stage pieces are passed over"""
    m = np.zeros(p.span, dtype=bool)
    for g, (e, rows) in enumerate(groups_of(p)):
        a, b = (1990, 2048) if g % 2 == 0 else (1600, 1700)
        m[e + min(a, rows):e + min(b, rows)] = True
        if rows > 64:
            m[e + 64] = True
    return m


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 37])
def test_every_mode_under_every_mask(adac, gpu_ctx, phase):
    rng = np.random.default_rng(1)
    v = kind_column(np.int32, rng, [g % 5 for g in range(25)])
    dev = Dev(adac, gpu_ctx, Packed(v, phase=phase))
    p = dev.p
    assert len(p.modes) == 26 and {m for m, _ in p.modes} >= {1, 2, 3, 4}, p.modes
    assert any(m == DELTA and w >= 1 for m, w in p.modes), p.modes
    assert p.span == phase + len(v)
    masks = four_masks(p.span, rng)
    masks["sparse"] = rng.random(p.span) < 1 / 500
    ends, late = np.zeros(p.span, dtype=bool), np.zeros(p.span, dtype=bool)
    for e, rows in groups_of(p):
        ends[e] = ends[e + rows - 1] = True
        late[e + 1984:e + rows] = True       # a DELTA_FOR prefix passes through 31 unselected steps first
    masks["ends"], masks["late"] = ends, late
    totals = {name: check_selected(dev, m) for name, m in masks.items()}
    assert totals["zero"] == 0 and totals["one"] == len(v)
    assert totals["ends"] == 2 * 26 and totals["late"] == 25 * 64
    assert totals["sparse"] > 0


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
def test_types(adac, gpu_ctx, dtype):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(10 + dtype.itemsize + (dtype.kind == "i"))
    dev = Dev(adac, gpu_ctx, Packed(kind_column(dtype, rng, [g % 5 for g in range(10)])))
    masks = four_masks(dev.p.span, rng)
    check_selected(dev, masks["random"])
    check_selected(dev, masks["steps"])


# 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [FOR, DELTA])
@pytest.mark.parametrize("signed", [False, True])
def test_64_bit_fields_wider_than_32_bits(adac, gpu_ctx, mode, signed):
    rng = np.random.default_rng(20 + mode + signed)
    dev = Dev(adac, gpu_ctx, Packed(wide64(rng, mode, signed), mode))
    assert all(m == mode and w > 32 for m, w in dev.p.modes[:-1]), dev.p.modes
    masks = four_masks(dev.p.span, rng)
    check_selected(dev, masks["random"])
    check_selected(dev, masks["steps"])
    check_selected(dev, far_window(dev.p))


@pytest.mark.parametrize("mode", [FOR, DELTA])
@pytest.mark.parametrize("w,dtype", [(16, np.uint32), (17, np.uint32), (21, np.int64), (40, np.uint64)])
def test_exact_widths_and_stage_pieces(adac, gpu_ctx, mode, w, dtype):
    rng = np.random.default_rng(30 + w + mode)
    if mode == DELTA and np.dtype(dtype).itemsize == 4:
        dtype = np.uint64   # 2048 deltas of 16 or 17 bits leave 32 bits
    dev = Dev(adac, gpu_ctx, Packed(width_values(rng, w, mode, dtype), mode))
    assert all(m == (mode, w) for m in dev.p.modes[:-1]), dev.p.modes
    masks = four_masks(dev.p.span, rng)
    check_selected(dev, masks["random"])
    check_selected(dev, masks["steps"])
    assert check_selected(dev, far_window(dev.p)) > 0


# 4 -----------------------------------------------------------------------------------------------------------------
def test_width_zero_for_and_delta_for(adac, gpu_ctx):
    """Forced FOR over constant groups and forced DELTA_FOR over an arithmetic progression: the width-0 forms."""
    rng = np.random.default_rng(2)
    const = np.repeat(np.arange(100, 106, dtype=np.int64), GROUP)[:5 * GROUP + 777].astype(np.int32)
    ramp = (50 + 3 * np.arange(5 * GROUP + 777, dtype=np.int64)).astype(np.int32)
    pc, pr = Packed(const, FOR), Packed(ramp, DELTA)
    assert all(m == (FOR, 0) for m in pc.modes), pc.modes
    assert all(m == DELTA for m, _ in pr.modes) and any(w == 0 for _, w in pr.modes), pr.modes
    for p in (pc, pr):
        dev = Dev(adac, gpu_ctx, p)
        for name, m in four_masks(p.span, rng).items():
            check_selected(dev, m)


# 5 -----------------------------------------------------------------------------------------------------------------
def test_segments_and_runs_of_groups_that_cross_their_ends(adac, gpu_ctx):
    rng = np.random.default_rng(40)
    n = 40 * GROUP + 777
    dev = Dev(adac, gpu_ctx, Packed(rng.integers(0, 1 << 62, size=n, dtype=np.uint64)))
    assert dev.p.nseg == 3
    mask = rng.random(n) < 0.5
    check_selected(dev, mask)
    adac.set_tuning("num_cus", 1)   # 32 waves for 41 groups: runs of two groups, one of them across a segment end
    try:
        check_selected(dev, mask)
        check_selected(dev, np.ones(n, dtype=bool))
    finally:
        adac.set_tuning("num_cus", 0)


def test_element_space_with_gaps(adac, gpu_ctx):
    rng = np.random.default_rng(50)
    counts = [3 * GROUP, 0, 2 * GROUP + 777]
    out_offs = [37, 37 + counts[0] + 50, 37 + counts[0] + 100]
    v = rng.integers(-(1 << 20), 1 << 20, size=sum(counts)).astype(np.int32)
    dev = Dev(adac, gpu_ctx, Packed(v, counts=counts, out_offs=out_offs))
    p = dev.p
    assert p.span == out_offs[2] + counts[2] and not p.cover[:37].any() and not p.cover[37 + counts[0]:out_offs[2]].any()
    assert all(o % 64 for o in out_offs)
    mask = rng.random(p.nwords * 64 + 64) < 0.5
    total = check_selected(dev, mask)
    noisy = mask.copy()                       # every bit no segment covers set: in the gaps and past the span
    noisy[:p.span][~p.cover] = True
    noisy[p.span:] = True
    assert check_selected(dev, noisy) == total
    quiet = mask.copy()
    quiet[:p.span][~p.cover] = False
    quiet[p.span:] = False
    assert check_selected(dev, quiet) == total
    assert check_selected(dev, np.ones(p.nwords * 64 + 64, dtype=bool)) == len(v)


def test_one_row_and_no_rows(adac, gpu_ctx):
    ctx = gpu_ctx
    one = Dev(adac, ctx, Packed(np.array([-7], dtype=np.int8)))
    assert check_selected(one, np.array([True])) == 1
    assert check_selected(one, np.array([False])) == 0
    # layouts of zero rows: total 0, nothing written, no pointer looked at
    zero = [Dev(adac, ctx, Packed(np.zeros(0, np.int32), counts=[0, 0])).lay,
            adac.BitpackingLayout(ctx, np.int32, np.zeros(0, np.uint64), np.zeros(0, np.uint32))]
    for lay in zero:
        d_out, d_ids, d_mask = fresh(ctx, 4), fresh(ctx, 4), fresh(ctx, 4)
        for _ in range(2):
            assert lay.unpack_selected(None, d_mask, d_out, d_ids) == 0
            assert lay.unpack_selected(None, None, None) == 0
            assert lay.unpack_selected(d_mask.ptr + 8, d_mask, d_out, want_total=False) is None
        ctx.sync()
        assert untouched(d_out, 4) and untouched(d_ids, 4)


# 6 -----------------------------------------------------------------------------------------------------------------
def test_after_a_select(adac, gpu_ctx):
    """filter -> project: the bitmap of adac_bp_scan_select_between on one column selects the rows of two others whose
    blocks end elsewhere; the element space is back to back."""
    ctx = gpu_ctx
    rng = np.random.default_rng(60)
    n = 40 * GROUP + 777
    key = rng.integers(-(1 << 30), 1 << 30, size=n).astype(np.int32)
    small = rng.integers(0, 200, size=n).astype(np.uint8)
    big = rng.integers(-(1 << 61), 1 << 61, size=n).astype(np.int64)
    dk, ds, db = (Dev(adac, ctx, Packed(x)) for x in (key, small, big))
    assert len({dk.p.nseg, ds.p.nseg, db.p.nseg}) == 3, (dk.p.nseg, ds.p.nseg, db.p.nseg)
    lo, hi = -(1 << 28), 1 << 29
    d_bitmap, d_counts = fresh(ctx, dk.p.nwords), fresh(ctx, dk.p.nseg)
    dk.lay.scan_select_between(dk.d_blocks, lo & 0xffffffff, hi & 0xffffffff, d_bitmap, d_counts)
    selected = int(d_counts.download(np.uint64, dk.p.nseg).sum())
    keep = (key >= lo) & (key <= hi)
    assert selected == int(keep.sum()) and 0 < selected < n
    for dev, col in ((ds, small), (db, big)):
        ts = col.dtype.itemsize
        for _ in range(2):
            d_out, d_ids = filled(ctx, n * ts + 8), filled(ctx, n * 8 + 8)
            assert dev.lay.unpack_selected(dev.d_blocks, d_bitmap, d_out, d_ids) == selected
            assert np.array_equal(d_out.download(col.dtype, selected), col[keep])
            assert np.array_equal(d_ids.download(np.uint64, selected), np.flatnonzero(keep).astype(np.uint64))
            assert np.all(d_out.download(np.uint8, (n - selected) * ts + 8, selected * ts) == 0xA5)
            assert np.all(d_ids.download(np.uint8, (n - selected) * 8 + 8, selected * 8) == 0xA5)


# 7 -----------------------------------------------------------------------------------------------------------------
def test_optional_outputs_and_argument_errors(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(70)
    dev = Dev(adac, ctx, Packed(kind_column(np.int16, rng, [g % 5 for g in range(5)])))
    mask = rng.random(dev.p.span) < 0.5
    check_selected(dev, mask, ids=False)
    check_selected(dev, mask, want_total=False)
    check_selected(dev, mask, ids=False, want_total=False)
    n, ts = dev.p.span, 2
    d_mask = ctx.upload(pack_bits(mask, dev.p.nwords))
    d_out, d_ids = filled(ctx, n * ts + 8), filled(ctx, n * 8 + 8)

    def rejected(call):
        with pytest.raises(adac.AdacError) as err:
            call()
        assert err.value.status == 1
        ctx.sync()
        assert np.all(d_out.download(np.uint8, n * ts + 8) == 0xA5)      # nothing was enqueued
        assert np.all(d_ids.download(np.uint8, n * 8 + 8) == 0xA5)

    rejected(lambda: dev.lay.unpack_selected(dev.d_blocks, None, d_out, d_ids))
    rejected(lambda: dev.lay.unpack_selected(dev.d_blocks.ptr + 8, d_mask, d_out, d_ids))
    rejected(lambda: dev.lay.unpack_selected(None, d_mask, d_out, d_ids))
    rejected(lambda: dev.lay.unpack_selected(dev.d_blocks, d_mask, None, d_ids))
    assert adac.lib().adac_bp_unpack_selected(None, dev.d_blocks.ptr, d_mask.ptr, d_out.ptr, d_ids.ptr, None) == 1
    check_selected(dev, mask)       # and the layout still answers


# 8 -----------------------------------------------------------------------------------------------------------------
FUZZ_SEEDS = [73_000 + i for i in range(32)]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_small_fuzz(adac, gpu_ctx, seed):
    """Columns of decision-edge parts, a kind per metadata group; lengths at the group edges plus a few groups; masks of
    density 0, 1/64, 1/2 and 1; elements no row covers hold junk."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(ALL[seed % len(ALL)])
    n = fz.FIXED_N[(seed // len(ALL) + seed) % len(fz.FIXED_N)] + GROUP * int(rng.integers(0, 4))
    ngr = (n + GROUP - 1) // GROUP
    kinds = [fz._kind_for(rng, int(t), dtype) for t in rng.choice(fz.CYCLE, size=ngr)]
    col = fz.draw_column(rng, dtype, n, kinds)
    phase = int(rng.integers(0, 128))
    p = Packed(col.values, col.force, validity=col.validity, phase=phase)
    assert p.span == phase + n
    dev = Dev(adac, gpu_ctx, p)
    for density in (0.0, 1 / 64, 0.5, 1.0):
        mask = rng.random(p.nwords * 64 + 64) < 0.5              # junk below the phase and past the span
        mask[phase:phase + n] = rng.random(n) < density
        total = check_selected(dev, mask)
        assert total == {0.0: 0, 1.0: n}.get(density, total), (seed, density)
