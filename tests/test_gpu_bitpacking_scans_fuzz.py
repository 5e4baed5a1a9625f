"""Seeded fuzz of the six scans on DuckDB BITPACKING blocks (adac_bp_scan_sum / _min_max / _count_between /
_select_between / _sum_product / _group_sum) over columns that sit on the decision edges of BitpackingState::Flush,
alone and in pairs, and the directed cases a fuzz cannot be trusted to hit: the grouped scan at the group counts where
the number of LDS bin copies changes, keys wider than a dword whose low dword is a valid key, 64-bit DELTA_FOR at the
widths around the one-dword prefix (26 | 27 and 32 | 33) with one whole step of largest fields, and columns of 1 to 2049
rows.

The columns, their placement, the masks, probes and keys of a seed come from tests/bp_fuzz_columns.py;
tests/test_bp_fuzz_census.py asserts on the CPU what the seed lists reach.  Conventions of the other scan tests: every
output pre-filled with 0xA5 plus a guard word, every call made twice, expected values from numpy over the oracle's scan
of the same blocks (Column.check_*, bp_pair_cases.check_*).  On top of that, wherever the mask selects no row that was
NULL at compress, the expected values are computed a second time from the ORIGINAL values (sums mod 2^64 after widening
by the type's signedness, min / max and comparisons in T), so a mistake the oracle's scan shared with the kernels would
show; and for columns of at most 5 000 rows the sums are computed a third time in Python integers and the numpy
reference is held against them before the device is compared with either.

Teeth: each of seven one-line arithmetic mutations of the two .inl files (the pair cursor's and bp_scan_group's
one-dword bound at 27 instead of 26, the key compared on its low dword, DELTA_FOR at width 0 without its frame, `<=`
for `<` in the FOR interval shortcut, the linear forms' step cut to 32 bits in either file) fails tests here; three of
them pass every older bitpacking scan test.  A parametrised case takes 0.15 s or less on an MI355X."""
import numpy as np
import pytest

import bp_fuzz_columns as fz
from bp_pair_cases import (GROUP, Dev, Packed, check_group_sum, check_sum_product, kind_column, want_group_sum,
                           want_sum_product, widen)
from oracle import bitpacking as bp
from test_gpu_bitpacking_scans import Column, bits_of

pytestmark = pytest.mark.gpu
M64 = fz.M64
DELTA, FOR = bp.MODE_DELTA_FOR, bp.MODE_FOR
PY_ROWS = 5000          # up to here the sums are recomputed in Python integers


# ---- expected values from the original rows -------------------------------------------------------------------------
def seg_ranges(counts):
    ends = np.cumsum(np.asarray(counts, dtype=np.int64))
    return [(int(e) - int(c), int(e)) for c, e in zip(counts, ends)]


def orig_sum_min_max(v, keep, ranges):
    info = np.iinfo(v.dtype)
    sums, mm = [], []
    for r0, r1 in ranges:
        live = v[r0:r1][keep[r0:r1]]
        sums.append(int(widen(live).sum(dtype=np.uint64)))
        mm += ([bits_of(live.min(), v.dtype), bits_of(live.max(), v.dtype)] if len(live)
               else [bits_of(info.max, v.dtype), bits_of(info.min, v.dtype)])
    return sums, mm


def orig_sum_product(a, b, keep, ranges):
    prod = widen(a) * widen(b)                   # uint64 arithmetic wraps
    return [int(prod[r0:r1][keep[r0:r1]].sum(dtype=np.uint64)) for r0, r1 in ranges]


def orig_group_sum(v, k, ngroups, keep):
    keys = k.view("u%d" % k.dtype.itemsize).astype(np.uint64)        # unsigned, of the key type's own width
    bins = np.minimum(keys, np.uint64(ngroups)).astype(np.int64)[keep]
    sums = np.zeros(ngroups + 1, dtype=np.uint64)
    np.add.at(sums, bins, widen(v)[keep])
    return [int(x) for x in sums], [int(x) for x in np.bincount(bins, minlength=ngroups + 1)]


def rows_of(mask, phase, n):
    return np.ones(n, dtype=bool) if mask is None else np.asarray(mask[phase:phase + n], dtype=bool)


def within(keep, *validities):
    """no selected row was NULL at compress in any of the columns"""
    return all(valid is None or not (keep & ~valid).any() for valid in validities)


# ---- the same sums in Python integers -------------------------------------------------------------------------------
def py_sums(v, keep, ranges):
    x = [int(t) for t in v]
    return [sum(x[r] for r in range(r0, r1) if keep[r]) & M64 for r0, r1 in ranges]


def py_sum_product(a, b, keep, ranges):
    x, y = [int(t) for t in a], [int(t) for t in b]
    return [sum(x[r] * y[r] for r in range(r0, r1) if keep[r]) & M64 for r0, r1 in ranges]


def py_group_sum(v, k, ngroups, keep):
    kmask = (1 << (8 * k.dtype.itemsize)) - 1
    sums, counts = [0] * (ngroups + 1), [0] * (ngroups + 1)
    for x, key, on in zip(v.tolist(), k.tolist(), keep.tolist()):
        if on:
            b = min(key & kmask, ngroups)
            sums[b] += x
            counts[b] += 1
    return [s & M64 for s in sums], counts


class one_cu:
    """One CU's worth of waves: every wave walks a run of groups, across segment ends."""

    def __init__(self, adac, on):
        self.adac, self.on = adac, on

    def __enter__(self):
        if self.on:
            self.adac.set_tuning("num_cus", 1)

    def __exit__(self, *exc):
        if self.on:
            self.adac.set_tuning("num_cus", 0)


# ---- single-column seeds --------------------------------------------------------------------------------------------
def check_single(col, v, validity, phase, mask, probes):
    """sum, min / max and the range scans of one column under one mask: device == numpy over the oracle's scan (inside
    Column.check_*), and both == the original rows where no selected row was NULL at compress"""
    n = len(v)
    keep = rows_of(mask, phase, n)
    ranges = seg_ranges([len(s) for s in col.segs])
    exact = within(keep, validity)
    decoded = np.concatenate(col.segs) if col.segs else np.zeros(0, v.dtype)
    if n <= PY_ROWS:
        assert orig_sum_min_max(decoded, keep, ranges)[0] == py_sums(decoded, keep, ranges)
    want_sum, want_mm = col.check_sum_min_max(mask)
    assert (want_sum, want_mm) == orig_sum_min_max(decoded, keep, ranges)
    if exact:
        assert (want_sum, want_mm) == orig_sum_min_max(v, keep, ranges)
    for lo, hi in probes:
        sel = col.check_range(lo, hi, mask)
        if exact:
            want = np.zeros(col.span, dtype=bool)
            want[phase:phase + n] = (v >= v.dtype.type(lo)) & (v <= v.dtype.type(hi)) & keep
            assert np.array_equal(sel, want), (lo, hi)


def run_single_seed(adac, ctx, seed):
    c = fz.single_case(seed)
    v = c.col.values
    col = Column.from_values(adac, ctx, v, c.col.force, validity=c.col.validity, phase=c.phase)
    assert col.span == c.phase + c.n
    with one_cu(adac, c.one_cu):
        for j, (name, mask) in enumerate(c.masks.items()):
            # every probe without a mask; under a mask the whole type and two of the others in turn
            probes = c.probes if mask is None else [c.probes[0], c.probes[1 + j % (len(c.probes) - 1)],
                                                    c.probes[1 + (j + 3) % (len(c.probes) - 1)]]
            try:
                check_single(col, v, c.col.validity, c.phase, mask, probes)
            except AssertionError as e:
                raise AssertionError("single seed %d (%s, %d rows, force %d, phase %d, one_cu %s), mask %s: %s"
                                     % (seed, v.dtype.name, c.n, c.col.force, c.phase, c.one_cu, name, e)) from e


SINGLE_BLOCKS = 8


@pytest.mark.parametrize("block", range(SINGLE_BLOCKS))
def test_single_column_scans_fuzz(adac, gpu_ctx, block):
    for seed in fz.SINGLE_SEEDS[block::SINGLE_BLOCKS]:
        run_single_seed(adac, gpu_ctx, seed)


# ---- pair seeds -----------------------------------------------------------------------------------------------------
def check_pair_product(da, db, va, vb, validities, phase, mask):
    """SUM(a * b) per segment of da under one mask; va, vb: the original rows"""
    a, b, n = da.p, db.p, len(va)
    keep = rows_of(mask, phase, n)
    ranges = seg_ranges(a.counts)
    ref = want_sum_product(a, b, mask)
    if n <= PY_ROWS:
        assert ref == py_sum_product(a.raw[phase:phase + n], b.raw[phase:phase + n], keep, ranges)
    assert check_sum_product(da, db, mask) == ref
    if within(keep, *validities):
        assert ref == orig_sum_product(va, vb, keep, ranges)


def check_pair_group(dv, dk, vv, vk, validities, phase, ngroups, mask, with_counts=True):
    v, k, n = dv.p, dk.p, len(vv)
    keep = rows_of(mask, phase, n)
    ref = want_group_sum(v, k, ngroups, mask)
    if n <= PY_ROWS:
        assert ref == py_group_sum(v.raw[phase:phase + n], k.raw[phase:phase + n], ngroups, keep)
    assert check_group_sum(dv, dk, ngroups, mask, with_counts=with_counts) == ref
    if within(keep, *validities):
        assert ref == orig_group_sum(vv, vk, ngroups, keep)
    return ref


def run_pair_seed(adac, ctx, seed):
    c = fz.pair_case(seed)
    a, b = c.a, c.b
    da = Dev(adac, ctx, Packed(a.values, a.force, validity=a.validity, phase=c.phase))
    db = Dev(adac, ctx, Packed(b.values, b.force, validity=b.validity, phase=c.phase))
    assert da.p.span == db.p.span == c.phase + c.n
    if c.b_is_key:      # almost every key is above ngroups; a signed key counts as an unsigned number of its own width
        dk, keys, key_valid = db, b.values, b.validity
    else:
        dk, keys, key_valid = Dev(adac, ctx, Packed(c.keys, phase=c.phase)), c.keys, None
    with one_cu(adac, c.one_cu):
        for name, mask in c.masks.items():
            try:
                check_pair_product(da, db, a.values, b.values, (a.validity, b.validity), c.phase, mask)
                check_pair_product(db, da, b.values, a.values, (a.validity, b.validity), c.phase, mask)
                check_pair_group(da, dk, a.values, keys, (a.validity, key_valid), c.phase, c.ngroups, mask)
                if name in ("none", "random"):
                    check_pair_group(da, dk, a.values, keys, (a.validity, key_valid), c.phase, c.ngroups, mask,
                                     with_counts=False)
            except AssertionError as e:
                raise AssertionError("pair seed %d (%s x %s, %d rows, force %d / %d, phase %d, one_cu %s, %d groups, "
                                     "key %s), mask %s: %s"
                                     % (seed, a.dtype.name, b.dtype.name, c.n, a.force, b.force, c.phase, c.one_cu,
                                        c.ngroups, "b" if c.b_is_key else c.ktype.name, name, e)) from e


PAIR_BLOCKS = 16


@pytest.mark.parametrize("block", range(PAIR_BLOCKS))
def test_pair_scans_fuzz(adac, gpu_ctx, block):
    for seed in fz.PAIR_SEEDS[block::PAIR_BLOCKS]:
        run_pair_seed(adac, gpu_ctx, seed)


# ---- (a) the grouped scan where the number of bin copies changes ----------------------------------------------------
@pytest.mark.parametrize("ngroups", [15, 16, 31, 32, 63, 64, 127, 128])
def test_group_sum_at_every_bin_copy_threshold(adac, gpu_ctx, ngroups):
    """ngroups + 1 bins in 16 / 8 / 4 / 2 / 1 copies: 16 | 17, 32 | 33, 64 | 65 and 128 | 129 bins.  Random keys, so
    every lane - every copy - adds rows: with one copy too many a bin's copies run into the next array."""
    rng = np.random.default_rng(900 + ngroups)
    n = 3 * GROUP + 100
    keys = rng.integers(0, ngroups + 2, size=n)
    keys[:ngroups + 2] = np.arange(ngroups + 2)                # every key 0 .. ngroups + 1 is there
    keys = keys.astype(np.uint16)
    vals = rng.integers(-(1 << 30), 1 << 30, size=n).astype(np.int32)
    vals[:2] = [-(1 << 30), (1 << 30) - 1]          # (max - min has to fit the signed type to be encodable)
    pk = Packed(keys)
    assert all(m == FOR for m, _ in pk.modes), pk.modes
    dv, dk = Dev(adac, gpu_ctx, Packed(vals)), Dev(adac, gpu_ctx, pk)
    for mask in (None, rng.random(n) < 0.5):
        keep = rows_of(mask, 0, n)
        sums, counts = check_pair_group(dv, dk, vals, keys, (), 0, ngroups, mask)
        assert min(counts[:ngroups]) > 0 and counts[ngroups] == int((keys[keep] >= ngroups).sum()) > 0
        check_pair_group(dv, dk, vals, keys, (), 0, ngroups, mask, with_counts=False)


# ---- (b) keys wider than a dword ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngroups", [6, 256])
@pytest.mark.parametrize("ktype", [np.uint64, np.int64])
def test_keys_wider_than_a_dword_whose_low_dword_is_a_key(adac, gpu_ctx, ktype, ngroups):
    """k + (j << 32), j >= 1: every such row belongs in the overflow entry, whatever its low dword says."""
    ktype = np.dtype(ktype)
    rng = np.random.default_rng(1000 + ngroups + (ktype.kind == "i"))
    n = 3 * GROUP + 100
    k = rng.integers(0, ngroups, size=n).astype(object)
    high = rng.integers(1, 1 << 12, size=n).astype(object) * (rng.random(n) < 0.5)
    keys = k + high * (1 << 32)                                              # FOR at a width above 32
    if ktype.kind == "i":
        keys[rng.random(n) < 0.05] = -1                                      # all ones: above every group count
        keys[3] = -1
    keys[GROUP:2 * GROUP] = 3 + (1 << 32)                                    # CONSTANT
    keys[2 * GROUP:3 * GROUP] = 5 + np.arange(GROUP).astype(object) * (1 << 32)   # CONSTANT_DELTA, step 2^32
    keys = np.array(keys.tolist(), dtype=ktype)
    pk = Packed(keys)
    assert [m for m, _ in pk.modes] == [FOR, bp.MODE_CONSTANT, bp.MODE_CONSTANT_DELTA, FOR], pk.modes
    assert pk.modes[0][1] > 32 and pk.modes[3][1] > 32, pk.modes
    vals = rng.integers(-(1 << 30), 1 << 30, size=n).astype(np.int32)
    dv, dk = Dev(adac, gpu_ctx, Packed(vals)), Dev(adac, gpu_ctx, pk)
    low_is_key = (keys.view(np.uint64) >= np.uint64(1 << 32)) & ((keys.view(np.uint64) & np.uint64(0xffffffff))
                                                                 < np.uint64(ngroups))
    for g in (0, 2, 3):          # in the FOR groups and in the CONSTANT_DELTA group
        assert low_is_key[g * GROUP:(g + 1) * GROUP].sum() > 30
    for mask in (None, rng.random(n) < 0.5):
        keep = rows_of(mask, 0, n)
        sums, counts = check_pair_group(dv, dk, vals, keys, (), 0, ngroups, mask)
        over = int((keys.view(np.uint64)[keep] >= np.uint64(ngroups)).sum())
        assert counts[ngroups] == over >= int(low_is_key[keep].sum())


# ---- (c), (d): all six entry points over one column -----------------------------------------------------------------
def check_all_six(adac, ctx, v, force, masks, probes, partner, keys, ngroups, expect=None):
    """v through sum, min / max, count / select between, SUM(v * partner) in both orders and with itself, grouped by
    `keys` and as the key column of `partner`; every expected value from the original rows too"""
    n = len(v)
    col = Column.from_values(adac, ctx, v, force)
    pv = Packed(v, force)
    if expect is not None:
        expect(pv.modes)
    dv, dp, dk = Dev(adac, ctx, pv), Dev(adac, ctx, Packed(partner)), Dev(adac, ctx, Packed(keys))
    for mask in masks:
        check_single(col, v, None, 0, mask, probes)
        for (x, vx), (y, vy) in (((dv, v), (dp, partner)), ((dp, partner), (dv, v)), ((dv, v), (dv, v))):
            check_pair_product(x, y, vx, vy, (), 0, mask)
        check_pair_group(dv, dk, v, keys, (), 0, ngroups, mask)
        check_pair_group(dp, dv, partner, v, (), 0, ngroups, mask, with_counts=mask is None)
    return pv


def steps_mask(rng, n):
    return np.repeat(rng.random((n + 63) // 64) < 0.5, 64)[:n]


def prefix_bound_column(rng, dtype, w, slope, n=3 * GROUP + 100):
    """2^50 + cumsum(f + slope), f in [0, 2^w): 2^w - 1 on rows 320 .. 383 of every group (one whole step of the scan:
    64 (2^26 - 1) = 2^32 - 64 is the largest sum one dword holds), 0 at row 7 (so the frame is exactly `slope`)."""
    f = rng.integers(0, 1 << w, size=n, dtype=np.uint64).astype(np.int64)
    for g in range(0, n, GROUP):
        f[g + 320:g + 384] = (1 << w) - 1
        f[g + 7] = 0
    return ((1 << 50) + np.cumsum(f + slope)).astype(dtype)


@pytest.mark.parametrize("w", [26, 27, 32, 33])
@pytest.mark.parametrize("dtype", [np.int64, np.uint64])
def test_delta_for_64_bit_at_the_one_dword_prefix_bound(adac, gpu_ctx, dtype, w):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1100 + w + (dtype.kind == "i"))
    slopes = [0, -(1 << (w - 1)), -((1 << w) + 12345)] if dtype.kind == "i" else [0, 5]
    n = 3 * GROUP + 100
    partner = kind_column(np.int32, rng, [0, 1, 2], tail=100)
    keys = rng.integers(0, 9, size=n).astype(np.uint8)

    def exactly_w(modes):
        assert modes == [(DELTA, w)] * 4, modes

    for slope in slopes:
        v = prefix_bound_column(rng, dtype, w, slope)
        masks = (None, rng.random(n) < 0.5, steps_mask(rng, n))
        probes = [(int(v.min()), int(v.max())), tuple(sorted((int(v[1000]), int(v[5000])))), (int(v[352]), int(v[352]))]
        for force in (bp.MODE_AUTO, DELTA):
            pv = check_all_six(adac, gpu_ctx, v, force, masks, probes, partner, keys, 6, expect=exactly_w)
            # the frame is the slope: negative for the two descending / mixed columns
            frames = [fr for _, _, _, _, _, fr, _ in fz.segment_groups(bp.Compressed(v, force_mode=force))]
            assert frames == [slope & M64] * 4 and pv.nseg == 1


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049])
def test_short_columns_through_all_six(adac, gpu_ctx, n):
    rng = np.random.default_rng(1200 + n)
    partner = rng.integers(-1000, 1000, size=n).astype(np.int16)
    keys = rng.integers(0, 9, size=n).astype(np.uint8)
    delta = (-5000 + np.cumsum(rng.integers(-3, 40, size=n))).astype(np.int32)
    noise = rng.integers(-(1 << 20), 1 << 20, size=n).astype(np.int32)
    if n > 1:
        noise[0], noise[-1] = -(1 << 20), (1 << 20) - 1
    masks = [None, rng.random(n) < 0.5, steps_mask(rng, n)]
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    masks.append(last)

    def is_delta(modes):     # forced: two rows would be CONSTANT_DELTA.  A group of one row has no delta (FOR, width 0)
        assert [m for m, _ in modes] == ([DELTA] if 2 <= n <= GROUP else [DELTA, FOR] if n > GROUP else [FOR]), modes
        assert n < 63 or modes[0][1] >= 5

    def is_for(modes):
        assert all(m == FOR for m, _ in modes), modes
        assert modes[0][1] == (21 if n > 1 else 0)

    for v, expect in ((delta, is_delta), (noise, is_for)):
        probes = [(int(v.min()), int(v.max())), (int(v[n // 2]), int(v[n // 2])),
                  tuple(sorted((int(v[0]), int(v[-1]))))]
        check_all_six(adac, gpu_ctx, v, DELTA if v is delta else FOR, masks, probes, partner, keys, 6,
                      expect=expect)
