"""adac_scan_select_compare / adac_scan_count_compare on random layouts: 1 .. 20 segments of 0 .. 5000 rows, a random
type, encode rule, padding and value offsets on each side, a mask of random density, a random cmp; b is drawn on its
own or derived from a (equal, +-1, a shifted frame) segment by segment.  Held against numpy over the original columns."""
import numpy as np
import pytest

import scan_compare_cases as sc
from scan_compare_cases import check_compare
from test_gpu_sum_product import encode_column, offsets_of, place_mask, segment_at_width

gpu = pytest.mark.gpu


def derived(rng, a_seg, btype, how):
    """b from a's values as mathematical integers, clipped into b's type"""
    info = np.iinfo(btype)
    if how == "equal":
        d = np.zeros(len(a_seg), dtype=np.int64)
    elif how == "near":
        d = rng.integers(-1, 2, size=len(a_seg))
    else:  # a shifted frame: the same fields from another base
        d = np.full(len(a_seg), int(rng.integers(-300, 301)), dtype=np.int64)
    vals = [min(max(int(x) + int(s), int(info.min)), int(info.max)) for x, s in zip(a_seg, d)]
    return np.array(vals, dtype=object).astype(btype) if vals else np.zeros(0, dtype=btype)


def fuzz_case(seed):
    rng = np.random.default_rng(5000 + seed)
    nseg = int(rng.integers(1, 21))
    counts = rng.integers(0, 5001, size=nseg).astype(np.uint32)
    if rng.random() < 0.3:
        counts[rng.integers(0, nseg)] = 0
    atype, btype = (np.dtype(sc.TYPES[int(rng.integers(0, 8))]) for _ in range(2))
    a_segs, b_segs = [], []
    for c in counts:
        c = int(c)
        a_seg = segment_at_width(rng, atype, c, int(rng.integers(1, 8 * atype.itemsize + 1)))
        how = ("own", "equal", "near", "shift")[int(rng.integers(0, 4))]
        if how == "own":
            b_seg = segment_at_width(rng, btype, c, int(rng.integers(1, 8 * btype.itemsize + 1)))
        else:
            b_seg = derived(rng, a_seg, btype, how)
        a_segs.append(a_seg)
        b_segs.append(b_seg)
    a, b = np.concatenate(a_segs), np.concatenate(b_segs)

    def offsets():
        if rng.random() < 0.5:
            return None
        gaps = rng.integers(0, 71, size=nseg)
        return np.cumsum(gaps + np.concatenate([[0], counts[:-1]])).astype(np.uint64)

    density = (None, 0.02, 0.5, 0.98)[int(rng.integers(0, 4))]
    keep = None if density is None else rng.random(len(a)) < density
    return dict(counts=counts, a=a, b=b, aoffs=offsets(), boffs=offsets(), keep=keep,
                arule=int(rng.integers(0, 2)), brule=int(rng.integers(0, 2)), apad=bool(rng.integers(0, 2)),
                bpad=bool(rng.integers(0, 2)), cmp=int(rng.integers(1, 7)))


@gpu
@pytest.mark.parametrize("seed", range(40))
def test_fuzz(adac, gpu_ctx, seed):
    k = fuzz_case(seed)
    alay, awords = encode_column(adac, gpu_ctx, k["a"], k["counts"], k["aoffs"], rule=k["arule"], pad=k["apad"])
    blay, bwords = encode_column(adac, gpu_ctx, k["b"], k["counts"], k["boffs"], rule=k["brule"], pad=k["bpad"])
    d_mask = None
    if k["keep"] is not None:
        d_mask = gpu_ctx.upload(place_mask(k["keep"], k["counts"], offsets_of(k["counts"], k["aoffs"]),
                                           int(alay.value_span)))
    what = (seed, alay.dtype.name, blay.dtype.name, k["cmp"])
    check_compare(gpu_ctx, k["a"], alay, awords, k["b"], blay, bwords, k["counts"], cmps=(k["cmp"],), keep=k["keep"],
                  d_mask=d_mask, val_offs=k["aoffs"], what=what)
