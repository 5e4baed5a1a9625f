"""adac_scan_group_sum_product_mapped on random columns: every seed of a fixed list draws the key and `a` types, the
segments (sizes just past a scan group among them), the key distribution, the encode rule, the domain, the copies knob,
ngroups and the map (mapped_cases.fuzz_draw), and `b` from a generator of its own (product_mapped_cases.fuzz_draw); the
call is held against the numpy reference of product_mapped_cases.py, twice, into poisoned outputs, masked and unmasked.
tests/test_group_product_mapped_forms.py holds on the CPU that these seeds reach all five kernel forms."""
import pytest

import mapped_cases as mc
import product_mapped_cases as pc
from test_gpu_scan_select_compare import half_mask
from test_gpu_sum_product import encode_column

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("masked", (False, True), ids=("unmasked", "masked"))
@pytest.mark.parametrize("seed", range(mc.FUZZ_SEEDS))
def test_fuzz(adac, gpu_ctx, seed, masked):
    rng, keys, a, b, counts, rule, pad, base, span, knob, ngroups, codes = pc.fuzz_draw(seed)
    klay, kwords = encode_column(adac, gpu_ctx, keys, counts, rule=rule, pad=pad)
    alay, awords = encode_column(adac, gpu_ctx, a, counts, rule=rule, pad=pad)
    blay, bwords = encode_column(adac, gpu_ctx, b, counts, rule=rule, pad=pad)
    what = (seed, keys.dtype.name, a.dtype.name, b.dtype.name, [int(c) for c in counts], hex(base), span, ngroups, knob,
            pc.product_forms(klay, base, span, alay, blay))
    keep = d_mask = None
    if masked:
        keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(klay.value_span), p=float(rng.uniform(0.1, 0.9)))
    adac.set_tuning("group_mapped_copies", knob)
    try:
        pc.check_product(gpu_ctx, keys, a, b, klay, kwords, alay, awords, blay, bwords, counts, codes, base, span, ngroups,
                         keep, d_mask, what, every_output=seed % 4 == 0, pad=seed & 0xFF)
    finally:
        adac.set_tuning("group_mapped_copies", 0)
        for buf in (d_mask, kwords, awords, bwords):
            if buf is not None:
                buf.free()
        for lay in (klay, alay, blay):
            lay.close()
