"""adac_scan_select_member / adac_scan_count_member / adac_scan_build_member on random columns: every seed draws a type,
segment counts, widths, the encode rule, a domain, the set's density and a mask; probe and build are held against the
numpy reference of scan_member_cases.py (twice each, into poisoned outputs)."""
import importlib

import numpy as np
import pytest

import scan_member_cases as sm
from scan_member_cases import check_build, check_member, kind, random_set
from test_gpu_scan_select_compare import half_mask
from test_gpu_sum_product import encode_column

gpu = pytest.mark.gpu
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")
COUNTS = (0, 1, 63, 64, 65, 257, 1000, 2049, 4097, 9000)
SEEDS = 40


def draw(seed):
    rng = np.random.default_rng(3000 + seed)
    dtype = np.dtype(sm.TYPES[int(rng.integers(0, len(sm.TYPES)))])
    tb = 8 * dtype.itemsize
    nseg = int(rng.integers(1, 7))
    counts = np.array([COUNTS[int(rng.integers(0, len(COUNTS)))] for _ in range(nseg)], dtype=np.uint32)
    if not counts.any():
        counts[0] = 257
    widths = [int(rng.integers(1, tb + 1)) for _ in range(nseg)]
    segs = [sm.segment_at_width(rng, dtype, int(c), w) if c >= 2 else sm.segment_at_width(rng, dtype, 2, w)[:int(c)]
            for c, w in zip(counts, widths)]
    vals = np.concatenate(segs)
    rule, pad = int(rng.integers(0, 2)), bool(rng.integers(0, 2))
    # the domain: around a row of the column (so that it meets a segment), or anywhere in the type
    bits = min(int(2 ** rng.uniform(0, 20.5)), 1 << tb)
    if rng.random() < 0.8:
        at = int(sm.biased(vals)[int(rng.integers(0, len(vals)))])
        dlo = at - int(rng.integers(0, bits))
    else:
        dlo = int(rng.integers(0, (1 << tb) - 1, dtype=np.uint64, endpoint=True))
    dlo = min(max(dlo, 0), (1 << tb) - bits)
    density = float(rng.choice([0.02, 0.5, 0.5, 0.98]))
    return rng, dtype, counts, vals, rule, pad, dlo ^ sm.sign_bit(dtype), bits, density


@gpu
def test_fuzz(adac, gpu_ctx):
    seen, selected = set(), 0
    for seed in range(SEEDS):
        rng, dtype, counts, vals, rule, pad, base, bits, density = draw(seed)
        lay, words = encode_column(adac, gpu_ctx, vals, counts, rule=rule, pad=pad)
        seen |= set(forms.member_form_groups(lay.get_descs(), kind(dtype), base, bits))
        set_words = random_set(rng, bits, density)
        what = (seed, dtype.name, [int(c) for c in counts], hex(base), bits)
        hit = check_member(gpu_ctx, vals, lay, words, counts, base, bits, set_words, what=what)
        selected += int(hit.sum())
        check_build(gpu_ctx, vals, lay, words, counts, base, bits, what=what)
        keep, d_mask = half_mask(gpu_ctx, rng, counts, None, int(lay.value_span), p=float(rng.uniform(0.1, 0.9)))
        check_member(gpu_ctx, vals, lay, words, counts, base, bits, set_words, keep, d_mask, what=what + ("masked",))
        check_build(gpu_ctx, vals, lay, words, counts, base, bits, keep, d_mask, what=what + ("masked build",))
        d_mask.free()
        words.free()
        lay.close()
    assert {"header", "walk-slice", "walk-direct", "staged-slice", "staged-direct"} <= seen, seen
    assert selected > 1000
