"""adac_bp_scan_group_sum: SUM(value), COUNT(*) GROUP BY key over two columns of DuckDB BITPACKING blocks walked in
step, under an optional selection bitmap.  Blocks from the oracle's compress, expected values from numpy over the
oracle's scan of the same blocks; outputs pre-filled with 0xA5 plus a guard word; every call made twice
(tests/bp_pair_cases.py)."""
import numpy as np
import pytest

from oracle import bitpacking as bp
from bp_pair_cases import (ALL, GROUP, Dev, Packed, check_group_sum, four_masks, fresh, kind_column, pack_bits,
                           untouched)

pytestmark = pytest.mark.gpu
N = 25 * GROUP + 777
M64 = (1 << 64) - 1


def value_column(dtype, seed):
    rng = np.random.default_rng(seed)
    return kind_column(dtype, rng, [g % 5 for g in range(25)])


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
def test_value_types(adac, gpu_ctx, dtype):
    rng = np.random.default_rng(100 + np.dtype(dtype).itemsize)
    dv = Dev(adac, gpu_ctx, Packed(value_column(dtype, 5)))
    dk = Dev(adac, gpu_ctx, Packed(rng.integers(0, 6, size=N).astype(np.uint8)))
    sums, counts = check_group_sum(dv, dk, 6)
    assert counts[6] == 0 and min(counts[:6]) > 0 and sum(counts) == N
    check_group_sum(dv, dk, 6, rng.random(N) < 0.5)


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ngroups", [1, 6, 256])
@pytest.mark.parametrize("ktype", [np.uint8, np.uint16, np.uint32, np.int8])
def test_ngroups_and_key_types(adac, gpu_ctx, ngroups, ktype):
    ktype = np.dtype(ktype)
    rng = np.random.default_rng(200 + ngroups + ktype.itemsize)
    top = min(ngroups + 3, int(np.iinfo(ktype).max) + 1)      # a few keys >= ngroups where the type has room
    if ktype.kind == "i":
        top = min(top, 60)                                    # max - min must fit the signed type to be encodable
    keys = rng.integers(0, top, size=N).astype(ktype)
    if ktype.kind == "i":
        keys[rng.random(N) < 0.1] = -3                        # negative keys: large unsigned numbers
        keys[17] = -60
    dv = Dev(adac, gpu_ctx, Packed(value_column(np.int32, 6)))
    dk = Dev(adac, gpu_ctx, Packed(keys))
    sums, counts = check_group_sum(dv, dk, ngroups)
    over = int((keys.view("u%d" % ktype.itemsize) >= ngroups).sum())
    assert counts[ngroups] == over
    if ktype.kind == "i" and ngroups <= 128:      # a negative int8 is 128 .. 255 as a number of its own width
        assert over >= int((keys < 0).sum()) > 0
    elif ktype.kind == "i":                        # with 256 groups those are entries of their own
        assert over == 0 and counts[253] == int((keys == -3).sum()) > 0 and counts[196] == 1
    if top > ngroups:
        assert over > 0
    check_group_sum(dv, dk, ngroups, rng.random(N) < 0.5)


# 3 -----------------------------------------------------------------------------------------------------------------
def key_columns(rng):
    sorted_keys = np.repeat(np.arange(26) % 7, GROUP)[:N].astype(np.uint8)          # one key per 2048-row group
    ramp = (np.arange(N) % GROUP // 8).astype(np.uint16)                             # 0 .. 255 in every group
    ramp1 = (np.arange(N) % GROUP % 256).astype(np.uint16)
    walk = np.concatenate([np.sort(rng.integers(0, 10, size=GROUP)) for _ in range(26)])[:N].astype(np.uint32)
    return {"constant": (sorted_keys, bp.MODE_AUTO, {bp.MODE_CONSTANT}),
            "constant_delta": ((np.arange(N) % GROUP).astype(np.uint16), bp.MODE_AUTO, {bp.MODE_CONSTANT_DELTA}),
            "delta_for": (walk, bp.MODE_AUTO, {bp.MODE_DELTA_FOR}),
            "for_width_0": (sorted_keys, bp.MODE_FOR, {bp.MODE_FOR}),
            "ramps": (ramp, bp.MODE_AUTO, None), "saw": (ramp1, bp.MODE_AUTO, None)}


@pytest.mark.parametrize("shape", ["constant", "constant_delta", "delta_for", "for_width_0", "ramps", "saw"])
@pytest.mark.parametrize("vtype", [np.int32, np.uint64])
def test_key_column_modes_under_every_mask(adac, gpu_ctx, shape, vtype):
    rng = np.random.default_rng(300)
    keys, force, modes = key_columns(rng)[shape]
    pk = Packed(keys, force)
    if modes is not None:
        assert {m for m, _ in pk.modes} == modes, pk.modes
    if shape == "for_width_0":
        assert all(w == 0 for _, w in pk.modes)
    dk = Dev(adac, gpu_ctx, pk)
    dv = Dev(adac, gpu_ctx, Packed(value_column(vtype, 7)))
    ngroups = 6 if shape != "constant_delta" else 256          # keys >= ngroups in every shape
    sums, counts = check_group_sum(dv, dk, ngroups)
    assert counts[ngroups] > 0 and sum(counts) == N
    for name, m in four_masks(N, rng).items():
        s, c = check_group_sum(dv, dk, ngroups, m)
        if name == "zero":
            assert not any(s) and not any(c)
        if name == "one":
            assert (s, c) == (sums, counts)
    check_group_sum(dv, dk, ngroups, rng.random(N) < 0.5, with_counts=False)
    check_group_sum(dv, dk, ngroups, None, with_counts=False)


# 4 -----------------------------------------------------------------------------------------------------------------
def test_segmentation_that_differs(adac, gpu_ctx):
    rng = np.random.default_rng(400)
    n = 40 * GROUP + 777
    wide = Dev(adac, gpu_ctx, Packed(rng.integers(0, 1 << 62, size=n, dtype=np.uint64)))
    narrow = Dev(adac, gpu_ctx, Packed(rng.integers(0, 8, size=n).astype(np.uint8)))
    assert wide.p.nseg == 3 and narrow.p.nseg == 1 and wide.p.nseg != narrow.p.nseg
    mask = rng.random(n) < 0.5
    check_group_sum(wide, narrow, 6)            # values in three segments, keys in one
    check_group_sum(wide, narrow, 6, mask)
    check_group_sum(narrow, wide, 256, mask)    # and the roles swapped: every key lands in the overflow entry
    adac.set_tuning("num_cus", 1)               # every wave walks a run of groups
    try:
        check_group_sum(wide, narrow, 6, mask)
    finally:
        adac.set_tuning("num_cus", 0)


def test_element_space_with_gaps(adac, gpu_ctx):
    rng = np.random.default_rng(410)
    counts = [3 * GROUP, 2 * GROUP + 777]
    out_offs = [37, 37 + counts[0] + 100]
    n = sum(counts)
    dv = Dev(adac, gpu_ctx, Packed(rng.integers(-(1 << 20), 1 << 20, size=n).astype(np.int32), counts=counts,
                                   out_offs=out_offs))
    dk = Dev(adac, gpu_ctx, Packed(rng.integers(0, 9, size=n).astype(np.uint8), counts=counts, out_offs=out_offs))
    mask = rng.random(dv.p.nwords * 64) < 0.5
    want = check_group_sum(dv, dk, 6, mask)
    noisy = mask.copy()
    noisy[:dv.p.span][~dv.p.cover] = True
    noisy[dv.p.span:] = True
    assert check_group_sum(dv, dk, 6, noisy) == want
    check_group_sum(dv, dk, 6)


# 5 -----------------------------------------------------------------------------------------------------------------
def test_identity_with_scan_sum(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(500)
    dv = Dev(adac, ctx, Packed(value_column(np.int64, 8)))
    dk = Dev(adac, ctx, Packed(rng.integers(0, 300, size=N).astype(np.uint16)))
    for ngroups, mask in ((6, None), (256, rng.random(N) < 0.3), (100, four_masks(N, rng)["steps"])):
        d_valid = None if mask is None else ctx.upload(pack_bits(mask, dv.p.nwords))
        d_sums, d_counts, d_total = fresh(ctx, ngroups + 1), fresh(ctx, ngroups + 1), fresh(ctx, dv.p.nseg)
        dv.lay.scan_group_sum(dv.d_blocks, dk.lay, dk.d_blocks, ngroups, d_sums, d_counts, d_valid)
        dv.lay.scan_sum(dv.d_blocks, d_total, d_valid)
        sums = d_sums.download(np.uint64, ngroups + 1)
        counts = d_counts.download(np.uint64, ngroups + 1)
        total = d_total.download(np.uint64, dv.p.nseg)
        assert int(counts.sum()) == (N if mask is None else int(mask.sum()))
        assert int(sums.sum(dtype=np.uint64)) == int(total.sum(dtype=np.uint64))


# 6 -----------------------------------------------------------------------------------------------------------------
def test_zero_rows_and_one_row(adac, gpu_ctx):
    ctx = gpu_ctx
    dz = Dev(adac, ctx, Packed(np.zeros(0, np.int32), counts=[0, 0]))
    assert check_group_sum(dz, dz, 6) == ([0] * 7, [0] * 7)       # both arrays are still written
    for _ in range(2):
        d_sums = fresh(ctx, 7)
        dz.lay.scan_group_sum(None, dz.lay, None, 6, d_sums)
        assert not d_sums.download(np.uint64, 7).any()
    d1 = Dev(adac, ctx, Packed(np.array([-7], dtype=np.int8)))
    d2 = Dev(adac, ctx, Packed(np.array([3], dtype=np.uint32)))
    s, c = check_group_sum(d1, d2, 6)
    assert s[3] == (-7) & M64 and c == [0, 0, 0, 1, 0, 0, 0]
    s, c = check_group_sum(d2, d1, 6)                                # the key -7 is 249 as a uint8
    assert s[6] == 3 and c[6] == 1
    check_group_sum(d1, d2, 6, np.array([False]))


def test_argument_errors_and_accepted_segmentations(adac, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(600)
    v = rng.integers(-5000, 5000, size=4873).astype(np.int32)
    k = rng.integers(0, 8, size=4873).astype(np.uint8)
    one = Dev(adac, ctx, Packed(v, counts=[4873]))
    same = Dev(adac, ctx, Packed(k, counts=[4873]))
    split = Dev(adac, ctx, Packed(k, counts=[3000, 1873]))           # the same rows, different groups
    short = Dev(adac, ctx, Packed(k[:2048], counts=[2048]))          # a different group count
    ctx2 = adac.Context(0)
    try:
        other = Dev(adac, ctx2, Packed(k, counts=[4873]))
        d_sums, d_counts = fresh(ctx, 258), fresh(ctx, 258)

        def rejected(call):
            with pytest.raises(adac.AdacError) as err:
                call()
            assert err.value.status == 1
            assert untouched(d_sums, 258) and untouched(d_counts, 258)      # nothing was enqueued

        gs = lambda dv, vb, dk, kb, ng, s=d_sums, c=d_counts: dv.lay.scan_group_sum(vb, dk.lay, kb, ng, s, c)  # noqa: E731
        rejected(lambda: gs(one, one.d_blocks, split, split.d_blocks, 6))
        rejected(lambda: gs(split, split.d_blocks, one, one.d_blocks, 6))
        rejected(lambda: gs(one, one.d_blocks, short, short.d_blocks, 6))
        rejected(lambda: gs(one, one.d_blocks, other, other.d_blocks, 6))
        rejected(lambda: gs(one, one.d_blocks.ptr + 8, same, same.d_blocks, 6))
        rejected(lambda: gs(one, one.d_blocks, same, same.d_blocks.ptr + 8, 6))
        rejected(lambda: gs(one, None, same, same.d_blocks, 6))
        twin = ctx.upload(one.p.buf)   # one layout object binds one buffer at a time: twice with two buffers is refused
        rejected(lambda: gs(one, one.d_blocks, one, twin, 6))
        rejected(lambda: gs(one, one.d_blocks, same, None, 6))
        rejected(lambda: gs(one, one.d_blocks, same, same.d_blocks, 6, None))
        rejected(lambda: gs(one, one.d_blocks, same, same.d_blocks, 0))
        rejected(lambda: gs(one, one.d_blocks, same, same.d_blocks, 257))
        L = adac.lib()
        assert L.adac_bp_scan_group_sum(None, one.d_blocks.ptr, same.lay._h, same.d_blocks.ptr, None, 6, d_sums.ptr,
                                        None) == 1
        assert L.adac_bp_scan_group_sum(one.lay._h, one.d_blocks.ptr, None, same.d_blocks.ptr, None, 6, d_sums.ptr,
                                        None) == 1
        assert untouched(d_sums, 258)
        check_group_sum(one, same, 6)
        check_group_sum(one, same, 256)
    finally:
        ctx2.close()
    x = Dev(adac, ctx, Packed(v, counts=[4096, 777]))
    y = Dev(adac, ctx, Packed(k, counts=[2048, 2825]))               # different segments, the same groups
    check_group_sum(x, y, 6, rng.random(4873) < 0.5)
    check_group_sum(x, y, 6)
