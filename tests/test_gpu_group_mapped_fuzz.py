"""adac_scan_group_sum_mapped / adac_scan_group_count_mapped / adac_scan_build_map on random columns: every seed of a fixed
list draws the two types, the segments (sizes just past a scan group among them), the key distribution, the encode rule,
the domain, a mask (dense_cases.fuzz_draw), then ngroups, the map (uniform codes, skewed to one code, mostly 255) and the
copies knob (mapped_cases.fuzz_draw); the entries are held against the numpy reference of mapped_cases.py, twice each,
into poisoned outputs.  The value column doubles as the codes column of a build over the same keys.
tests/test_group_mapped_forms.py holds on the CPU that these seeds reach all five kernel forms."""
import numpy as np
import pytest

import mapped_cases as mc
from test_gpu_scan_select_compare import half_mask
from test_gpu_sum_product import encode_column

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("block", range(4))
def test_fuzz(adac, gpu_ctx, block):
    seen, rows = set(), 0
    per = mc.FUZZ_SEEDS // 4
    try:
        for seed in range(block * per, (block + 1) * per):
            rng, keys, vals, counts, rule, pad, base, span, knob, ngroups, codes = mc.fuzz_draw(seed)
            klay, kwords = encode_column(adac, gpu_ctx, keys, counts, rule=rule, pad=pad)
            vlay, vwords = encode_column(adac, gpu_ctx, vals, counts, rule=rule, pad=pad)
            seen |= set(mc.mapped_forms(klay, base, span, vlay)) | set(mc.mapped_forms(klay, base, span))
            adac.set_tuning("group_mapped_copies", knob)
            what = (seed, keys.dtype.name, vals.dtype.name, [int(c) for c in counts], hex(base), span, ngroups, knob)
            _, _, inside = mc.check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span,
                                           ngroups, what=what, pad=seed & 0xFF)
            rows += int(inside.sum())
            keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span), p=float(rng.uniform(0.1, 0.9)))
            mc.check_mapped(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, codes, base, span, ngroups, keep,
                            d_mask, what + ("masked",))
            mc.check_build(gpu_ctx, keys, vals, klay, kwords, vlay, vwords, counts, base, span, seed % 2 * 255, keep, d_mask,
                           what + ("build",))
            for b in (d_mask, kwords, vwords):
                b.free()
            klay.close()
            vlay.close()
    finally:
        adac.set_tuning("group_mapped_copies", 0)
    assert len(seen - {None}) >= 2 and rows > 0, (seen, rows)
