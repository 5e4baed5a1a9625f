"""Seeded fuzz of adac_bp_scan_select_compare / adac_bp_scan_count_compare over the pair seeds of
tests/bp_fuzz_columns.py: every fourth seed of PAIR_SEEDS, 40 seeds, none skipped.  The two columns of a seed sit on the
decision edges of BitpackingState::Flush, their types are drawn independently (mixed widths and signedness), and the
columns, the phase, the masks (random junk on elements no row covers) and one_cu are the seed's, treated as
tests/test_gpu_bitpacking_scans_fuzz.py treats them.  Per seed: all six comparisons under one of its masks, one
comparison drawn from the seed under every mask, the count form beside the select form every time.

Expected values: numpy over the oracle's scan of the same blocks, compared as Python integers (bp_compare_cases); and
wherever the mask selects no row that was NULL at compress, a second time from the ORIGINAL rows.  Conventions of
tests/bp_pair_cases.py: outputs pre-filled with 0xA5 plus a guard word, every call twice, every bitmap word compared."""
import numpy as np
import pytest

import bp_fuzz_columns as fz
from bp_compare_cases import ALL_CMPS, EQ, GT, LT, check_select_compare, relation
from bp_pair_cases import Dev, Packed

pytestmark = pytest.mark.gpu

SEEDS = fz.PAIR_SEEDS[::4]
BLOCKS = 8
assert len(SEEDS) == 40


def rows_of(mask, phase, n):
    return np.ones(n, dtype=bool) if mask is None else np.asarray(mask[phase:phase + n], dtype=bool)


def check_seed_compare(da, db, va, vb, validities, phase, cmp, mask, rel, orig_rel):
    bits, counts, _ = check_select_compare(da, db, cmp, mask, rel=rel)
    n = len(va)
    keep = rows_of(mask, phase, n)
    if all(valid is None or not (keep & ~valid).any() for valid in validities):
        assert np.array_equal(bits[phase:phase + n], keep & ((orig_rel & np.uint8(cmp)) != 0)), "original rows"
    assert not bits[:phase].any() and sum(counts) == int(bits.sum())


def run_seed(adac, ctx, seed):
    c = fz.pair_case(seed)
    a, b = c.a, c.b
    da = Dev(adac, ctx, Packed(a.values, a.force, validity=a.validity, phase=c.phase))
    db = Dev(adac, ctx, Packed(b.values, b.force, validity=b.validity, phase=c.phase))
    assert da.p.span == db.p.span == c.phase + c.n
    rel = relation(da.p, db.p)
    x, y = a.values.astype(object), b.values.astype(object)
    orig_rel = np.where(np.asarray(x < y, dtype=bool), LT, np.where(np.asarray(x == y, dtype=bool), EQ, GT)).astype(np.uint8)
    names = list(c.masks)
    all_six_under = names[seed // 4 % len(names)]
    one_cmp = ALL_CMPS[seed // 4 % len(ALL_CMPS)]
    adac.set_tuning("num_cus", 1 if c.one_cu else 0)
    try:
        for name, mask in c.masks.items():
            for cmp in (ALL_CMPS if name == all_six_under else [one_cmp]):
                try:
                    check_seed_compare(da, db, a.values, b.values, (a.validity, b.validity), c.phase, cmp, mask, rel,
                                       orig_rel)
                except AssertionError as e:
                    raise AssertionError("pair seed %d (%s x %s, %d rows, force %d / %d, phase %d, one_cu %s), cmp %d, "
                                         "mask %s: %s" % (seed, a.dtype.name, b.dtype.name, c.n, a.force, b.force,
                                                          c.phase, c.one_cu, cmp, name, e)) from e
    finally:
        adac.set_tuning("num_cus", 0)


@pytest.mark.parametrize("block", range(BLOCKS))
def test_select_compare_fuzz(adac, gpu_ctx, block):
    for seed in SEEDS[block::BLOCKS]:
        run_seed(adac, gpu_ctx, seed)
