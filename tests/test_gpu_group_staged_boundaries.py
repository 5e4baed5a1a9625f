"""The stage arithmetic that the four generic (staged-LDS) grouped kernels each carry a copy of (next_stage in
k_group_sum, k_group_product, k_group_product3, k_group_q1), at the smallest shapes where it can go wrong: ONE segment
whose row count is one stage exactly, one stage + 1 and two stages + 1.

A stage holds ((3584 * 8 - 256) / widest width) & ~255 rows, at most 8192:
  * widest column at 64 bits: 256 rows per stage -> 256, 257 and 513 rows (`a` is a uint64 column: 2048 rows per tile);
  * every column at 1 bit: the 8192-row cap decides -> 8192 and 8193 rows (`a` is a uint8 column: 16384 rows per tile).
    The unmasked k_group_sum alone has no cap: its stage would be 28416 rows, so it also runs at 28417 rows (there the
    tile ends the stage first, after 16384 rows).
All four entry points with the register walk knobbed off (and at 257 bins, where it never runs), with and without a mask
whose first bit sits at bit 37 of its word (val_off = 37), at ngroups = 3 and ngroups = 256.  Expected: numpy over the
original columns, mod 2^64 (test_gpu_group_sum_q1.reference_q1), compared exactly."""
import numpy as np
import pytest

from test_gpu_group_sum_product import Col
from test_gpu_group_sum_q1 import COUNT, SUM_A, SUM_AB, SUM_ABC, TERMS, reference_q1
from test_gpu_group_sum_valid import element_mask
from test_gpu_sum_product import segment_at_width

pytestmark = pytest.mark.gpu

KNOBS = ["group_sum_rw", "group_product_rw", "group_product3_rw", "group_q1_rw"]
VAL_OFF = 37
FF = 0xFFFFFFFFFFFFFFFF
# widest width -> (type, width) of a, b, c, q
COLUMNS = {
    64: [(np.uint64, 64), (np.int32, 17), (np.uint16, 9), (np.int64, 33)],
    1: [(np.uint8, 1), (np.int16, 1), (np.uint32, 1), (np.int8, 1)],
}
STAGE_ROWS = {64: 256, 1: 8192}
assert all(((3584 * 8 - 256) // w) & ~255 >= STAGE_ROWS[w] and STAGE_ROWS[w] <= 8192 for w in STAGE_ROWS)


@pytest.fixture
def staged_only(adac):
    for k in KNOBS:
        adac.set_tuning(k, 0)
    yield
    for k in KNOBS:
        adac.set_tuning(k, 1)


def keys_for(rng, n, ngroups, wmax):
    """uint16 keys that hit real bins and the overflow bin: two values at width 1, else 0 .. ngroups + 44"""
    if wmax == 1:
        k = rng.integers(ngroups - 1, ngroups, size=n, endpoint=True).astype(np.uint16)
        k[0], k[n - 1] = ngroups - 1, ngroups
    else:
        k = rng.integers(0, ngroups + 44, size=n, endpoint=True).astype(np.uint16)
        k[0], k[n - 1] = 0, ngroups + 44
    return k


def run_case(adac, ctx, wmax, rows, entry_points, seed):
    rng = np.random.default_rng(seed)
    counts = [rows]
    offs = np.array([VAL_OFF], dtype=np.uint64)
    vals = [segment_at_width(rng, t, rows, w) for t, w in COLUMNS[wmax]]
    a = Col(adac, ctx, vals[0], counts, offs)   # the mask lives in a's element space: bit VAL_OFF + row
    b, c, q = (Col(adac, ctx, v, counts) for v in vals[1:])
    assert [x.widths() for x in (a, b, c, q)] == [[w] for _, w in COLUMNS[wmax]]
    keep = rng.random(rows) < 0.6
    keep[0], keep[rows - 1], keep[STAGE_ROWS[wmax] - 1] = True, True, False
    d_keep = ctx.upload(element_mask(keep, counts, offs, int(a.lay.value_span)))
    for ngroups in (3, 256):
        k = Col(adac, ctx, keys_for(rng, rows, ngroups, wmax), counts)
        assert max(k.widths() + [w for _, w in COLUMNS[wmax]]) == wmax
        n = ngroups + 1
        d_out, d_cnt = ctx.alloc((TERMS * n + 1) * 8), ctx.alloc(n * 8)
        for d_mask, kept in ((None, None), (d_keep, keep)):
            exp = reference_q1(a.vals, b.vals, c.vals, q.vals, k.vals, ngroups, kept)   # once for the four calls
            assert sum(exp[COUNT]) == (rows if kept is None else int(kept.sum()))

            def pair(call):
                d_out.upload(np.full(TERMS * n + 1, FF, dtype=np.uint64))
                d_cnt.upload(np.full(n, FF, dtype=np.uint64))
                call()
                return d_out.download(np.uint64, n).tolist(), d_cnt.download(np.uint64, n).tolist()

            what = (wmax, rows, ngroups, "masked" if kept is not None else "unmasked")
            if "sum" in entry_points:
                got = pair(lambda: a.lay.scan_group_sum_valid(a.words, k.lay, k.words, d_mask, ngroups, d_out, d_cnt))
                assert got == (exp[SUM_A], exp[COUNT]), ("group_sum",) + what
            if "product" in entry_points:
                got = pair(lambda: a.lay.scan_group_sum_product(a.words, b.lay, b.words, k.lay, k.words, ngroups, d_out,
                                                                d_cnt, d_mask))
                assert got == (exp[SUM_AB], exp[COUNT]), ("group_sum_product",) + what
            if "product3" in entry_points:
                got = pair(lambda: a.lay.scan_group_sum_product3(a.words, b.lay, b.words, c.lay, c.words, k.lay, k.words,
                                                                 ngroups, d_out, d_cnt, d_mask))
                assert got == (exp[SUM_ABC], exp[COUNT]), ("group_sum_product3",) + what
            if "q1" in entry_points:
                d_out.upload(np.full(TERMS * n + 1, FF, dtype=np.uint64))
                a.lay.scan_group_sum_q1(a.words, b.lay, b.words, c.lay, c.words, q.lay, q.words, k.lay, k.words, ngroups,
                                        d_out, d_mask)
                out = d_out.download(np.uint64, TERMS * n + 1)
                assert int(out[TERMS * n]) == FF   # nothing past the results
                assert out[:TERMS * n].reshape(TERMS, n).tolist() == exp, ("group_sum_q1",) + what
            assert a.lay.debug_group_handover() == 0   # the register walk did not run
        d_out.free()
        d_cnt.free()
    d_keep.free()


ALL_FOUR = ("sum", "product", "product3", "q1")


@pytest.mark.parametrize("wmax,rows", [(64, 256), (64, 257), (64, 513), (1, 8192), (1, 8193)])
def test_one_stage_one_more_and_two_stages_and_one(adac, gpu_ctx, staged_only, wmax, rows):
    run_case(adac, gpu_ctx, wmax, rows, ALL_FOUR, seed=1000 * wmax + rows)


def test_group_sum_past_its_uncapped_unmasked_stage(adac, gpu_ctx, staged_only):
    """28416 rows would fit one unmasked stage of k_group_sum at 1 bit; the masked form cuts at 8192"""
    run_case(adac, gpu_ctx, 1, 28417, ("sum",), seed=28417)
