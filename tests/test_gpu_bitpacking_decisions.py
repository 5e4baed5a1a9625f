"""Device BITPACKING compress (adac_bp_plan_create + adac_bp_write) against the hand-pinned decision table
(tests/bp_decision_cases.py), at every width of every type under forced modes, and at the 256 KiB block boundary:
refusal, byte-identical block images, the mode and width read back from the device's own image, and decode by
full scan, by ranges starting inside groups and by point fetch."""
import numpy as np
import pytest

import bp_decision_cases as T
from oracle import bitpacking as bp
from test_gpu_bitpacking import assert_blocks_equal_oracle, gpu_compress

pytestmark = pytest.mark.gpu


def device_groups(plan, d_blocks, dtype):
    """(mode, width) of every group, parsed from the device image: the uint64 at byte 0 points past the first
    group's metadata entry; entry g is the uint32 `data_off | mode << 24` at first - 4(g+1); FOR / DELTA_FOR
    headers are T frame, T width (adac_bitpacking.inl, top of file)."""
    ts = np.dtype(dtype).itemsize
    img = d_blocks.download(np.uint8, plan.nseg * plan.BLOCK_STRIDE)
    out = []
    for i in range(plan.nseg):
        _, count, size = plan.segment(i)
        blk = img[i * plan.BLOCK_STRIDE:i * plan.BLOCK_STRIDE + size]
        first = int(blk[:8].view(np.uint64)[0])
        for g in range((count + T.GROUP - 1) // T.GROUP):
            enc = int(blk[first - 4 * (g + 1):first - 4 * g].view(np.uint32)[0])
            mode, off = enc >> 24, enc & 0xFFFFFF
            out.append((mode, int(blk[off + ts]) if mode in (T.FOR, T.DELTA_FOR) else 0))
    return out


def check_decode(adac, ctx, plan, d_blocks, v, valid, starts=(1, 31, 32, 1000, 2047)):
    """full unpack, unpack_range from inside groups (and across segment ends), fetch_rows at the same rows"""
    dtype = v.dtype
    ok = np.ones(len(v), bool) if valid is None else valid
    segs = [plan.segment(i) for i in range(plan.nseg)]
    counts = np.array([c for _, c, _ in segs], dtype=np.uint32)
    lay = adac.BitpackingLayout(ctx, dtype, np.arange(plan.nseg, dtype=np.uint64) * plan.BLOCK_STRIDE, counts)
    d_out = ctx.alloc(len(v) * dtype.itemsize + 64)
    lay.unpack(d_blocks, d_out)
    got = d_out.download(dtype, len(v))
    assert np.array_equal(got[ok], v[ok]), "full scan"
    rows_abs, fseg, frow = [], [], []
    for i, (s0, c, _) in enumerate(segs):
        for st in sorted(set(list(starts) + [c - 1]) | {x + T.GROUP for x in starts}):
            if st >= c:
                continue
            cnt = min(c - st, 2 * T.GROUP + 5)
            d_r = ctx.alloc(cnt * dtype.itemsize + 64)
            lay.unpack_range(d_blocks, i, st, cnt, d_r)
            r = d_r.download(dtype, cnt)
            k = ok[s0 + st:s0 + st + cnt]
            assert np.array_equal(r[k], v[s0 + st:s0 + st + cnt][k]), ("range", i, st, cnt)
            rows_abs.append(s0 + st)
            fseg.append(i)
            frow.append(st)
    n = len(rows_abs)
    d_f = ctx.alloc(n * dtype.itemsize + 64)
    lay.fetch_rows(d_blocks, ctx.upload(np.array(fseg, np.uint32)), ctx.upload(np.array(frow, np.uint32)), n, d_f)
    f = d_f.download(dtype, n)
    rows_abs = np.array(rows_abs)
    k = ok[rows_abs]
    assert np.array_equal(f[k], v[rows_abs][k]), "fetch"


def oracle_or_none(v, valid, mode):
    try:
        return bp.Compressed(v, valid, mode, null_zero=valid is not None)
    except ValueError:
        return None


COLUMNS = T.columns()


@pytest.mark.parametrize("col", COLUMNS, ids=[k for k, _, _ in COLUMNS])
def test_decision_table_on_device(adac, gpu_ctx, col):
    _, case, pinned = col
    v, valid = case.values, case.valid
    for mode in T.MODES:
        comp = oracle_or_none(v, valid, mode)
        plan, d_blocks, _ = gpu_compress(adac, gpu_ctx, v, valid, mode)
        assert plan.encodable == (comp is not None), mode
        if mode in pinned:
            assert plan.encodable == (pinned[mode] is not T.REFUSED), (mode, case.cite)
        if comp is None:
            assert plan.nseg == 0 and d_blocks is None
            continue
        assert_blocks_equal_oracle(plan, d_blocks, comp)
        if mode in pinned:
            assert device_groups(plan, d_blocks, v.dtype) == pinned[mode], (mode, case.cite)
        check_decode(adac, gpu_ctx, plan, d_blocks, v, valid)


@pytest.mark.parametrize("dtype", T.ALL, ids=[np.dtype(d).name for d in T.ALL])
def test_width_sweep_on_device(adac, gpu_ctx, dtype):
    """FOR at every span width 0 .. B (with the GetEffectiveWidth jump), DELTA_FOR at every delta width with
    ascending and with descending deltas.  u8 / i8 / u16 / i16 group payloads start at odd or 2-byte offsets:
    k_bp_write's byte-copy branch."""
    sweeps = [(T.for_sweep(dtype, seed=1), T.FOR)] + \
        [(T.delta_for_sweep(dtype, desc, seed=2 + desc), T.DELTA_FOR) for desc in (False, True)]
    for (v, exp), mode in sweeps:
        plan, d_blocks, _ = gpu_compress(adac, gpu_ctx, v, None, mode)
        assert plan.encodable
        assert_blocks_equal_oracle(plan, d_blocks, bp.Compressed(v, force_mode=mode))
        assert device_groups(plan, d_blocks, v.dtype) == exp, mode
        check_decode(adac, gpu_ctx, plan, d_blocks, v, None, starts=(1, 31, 32, 1000, 2047, 5000))


@pytest.mark.parametrize("dtype,short", T.FILL_SHAPES, ids=["%s-%d" % (np.dtype(d).name, s) for d, s in T.FILL_SHAPES])
def test_block_fill_boundary_on_device(adac, gpu_ctx, dtype, short):
    """A block filled to 0 bytes of slack, or missed by `short` bytes (meta_ptr - data_ptr < bytes + 4,
    FlushAndCreateSegmentIfFull): segments equal the oracle and the hand model; decode across the boundary."""
    v, groups, b = T.fill_shape(dtype, short)
    segs, slack = T.place(dtype, groups)
    assert slack[b] == -short and len(segs) == 2
    plan, d_blocks, _ = gpu_compress(adac, gpu_ctx, v)
    comp = bp.Compressed(v)
    assert [plan.segment(i) for i in range(plan.nseg)] == segs
    assert_blocks_equal_oracle(plan, d_blocks, comp)
    assert device_groups(plan, d_blocks, v.dtype) == [(m, w) for _, m, w in groups]
    c0 = segs[0][1]
    check_decode(adac, gpu_ctx, plan, d_blocks, v, None, starts=(1, c0 - T.GROUP + 1, c0 - 1))
    # the last row of segment 0 and the first of segment 1, by range and by fetch
    lay = adac.BitpackingLayout(gpu_ctx, v.dtype, np.arange(2, dtype=np.uint64) * plan.BLOCK_STRIDE,
                                np.array([segs[0][1], segs[1][1]], dtype=np.uint32))
    d_r = gpu_ctx.alloc(64)
    lay.unpack_range(d_blocks, 0, c0 - 1, 1, d_r)
    lay.unpack_range(d_blocks, 1, 0, 1, d_r, 1)
    assert np.array_equal(d_r.download(v.dtype, 2), v[c0 - 1:c0 + 1])
    d_f = gpu_ctx.alloc(64)
    lay.fetch_rows(d_blocks, gpu_ctx.upload(np.array([0, 1], np.uint32)),
                   gpu_ctx.upload(np.array([c0 - 1, 0], np.uint32)), 2, d_f)
    assert np.array_equal(d_f.download(v.dtype, 2), v[c0 - 1:c0 + 1])
