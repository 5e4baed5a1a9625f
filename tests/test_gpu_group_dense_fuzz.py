"""adac_scan_group_sum_dense / adac_scan_group_count_dense on random columns: every seed of a fixed list draws the two
types, the segments (sizes just past a scan group among them), the key distribution (sorted, clustered, uniform), the
encode rule, the domain, a mask and the run-combining knob (dense_cases.fuzz_draw); both entries are held against the
numpy reference of dense_cases.py, twice each, into poisoned outputs.  tests/test_group_dense_forms.py holds on the CPU
that these seeds reach all five kernel forms."""
import numpy as np
import pytest

import dense_cases as dc
from test_gpu_scan_select_compare import half_mask
from test_gpu_sum_product import encode_column

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("block", range(4))
def test_fuzz(adac, gpu_ctx, block):
    seen, rows = set(), 0
    per = dc.FUZZ_SEEDS // 4
    try:
        for seed in range(block * per, (block + 1) * per):
            rng, keys, vals, counts, rule, pad, base, span, combine = dc.fuzz_draw(seed)
            klay, kwords = encode_column(adac, gpu_ctx, keys, counts, rule=rule, pad=pad)
            vlay, vwords = encode_column(adac, gpu_ctx, vals, counts, rule=rule, pad=pad)
            seen |= set(dc.dense_forms(klay, base, span, vlay)) | set(dc.dense_forms(klay, base, span))
            adac.set_tuning("group_dense_combine", combine)
            what = (seed, keys.dtype.name, vals.dtype.name, [int(c) for c in counts], hex(base), span, combine)
            _, _, inside = dc.check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, what=what)
            rows += int(inside.sum())
            keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span), p=float(rng.uniform(0.1, 0.9)))
            dc.check_dense(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, keep, d_mask,
                           what + ("masked",))
            for b in (d_mask, kwords, vwords):
                b.free()
            klay.close()
            vlay.close()
    finally:
        adac.set_tuning("group_dense_combine", 1)
    assert len(seen - {None}) >= 2 and rows > 0, (seen, rows)
