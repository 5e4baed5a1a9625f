"""forms.dense_form_groups (the host mirror of dense_plan, csrc/adac_group_dense.inl) against the rule written once more
with Python integers over the MATHEMATICAL values, and the columns of the GPU tests held on the CPU: the fuzz's fixed
seeds reach every one of the five forms.  Without this the GPU tests could pass on columns that never leave one form."""
import importlib
import os

import numpy as np
import pytest

import dense_cases as dc
import scan_compare_cases as sc
import scan_member_cases as sm

adac = importlib.import_module("duckdb-adaptive-compression_amd")
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_MIN = 0xFFFFFFFFFFFFFFFF
W = forms.DENSE_WINDOW


def seg(width, vmin=0, count=1000, packed=True):
    d = np.zeros(1, dtype=adac.SEGMENT_DESC_DTYPE)
    d["count"], d["width"], d["flags"] = count, width, 1 if packed else 0
    d["min"] = NO_MIN if vmin is None else vmin & NO_MIN
    return d


def as_value(pattern, size, signed):
    """a zero-extended bit pattern of the type as the mathematical integer it stands for"""
    tb = 8 * size
    pattern &= (1 << tb) - 1
    return pattern - (1 << tb) if signed and pattern >> (tb - 1) else pattern


def interval(d, size, signed):
    """[first, last] of the values a segment can hold when value = field + frame never leaves the type, else None"""
    tb, w = 8 * size, int(d["width"][0])
    tmax = (1 << (tb - 1)) - 1 if signed else (1 << tb) - 1
    if int(d["flags"][0]) & 1 and int(d["min"][0]) != NO_MIN:
        first = as_value(int(d["min"][0]), size, signed)
        return (first, first + (1 << w) - 1) if first + (1 << w) - 1 <= tmax else None
    return None if signed else (0, (1 << w) - 1)


def brute(d, k_type, base, span, dv=None, v_type=None):
    if int(d["count"][0]) == 0:
        return None
    iv = interval(d, *k_type)
    if iv is None:
        return "staged-direct"
    lo = as_value(base, *k_type)
    hi = lo + span - 1
    if iv[1] < lo or hi < iv[0]:
        return "header"
    reach = min(iv[1], hi) - max(iv[0], lo) + 1

    def walkable(x, t, wmin):
        w = int(x["width"][0])
        return wmin <= w <= 32 and int(x["count"][0]) * w < 2 ** 31 and interval(x, *t) is not None
    walk = walkable(d, k_type, 4) and (dv is None or walkable(dv, v_type, 1))
    return ("walk" if walk else "staged") + ("-window" if reach <= W else "-direct")


def type_ends(size, signed):
    tb = 8 * size
    return (-(1 << (tb - 1)), (1 << (tb - 1)) - 1) if signed else (0, (1 << tb) - 1)


def test_the_window_is_the_kernels():
    src = open(os.path.join(ROOT, "duckdb-adaptive-compression_amd", "csrc", "adac_group_dense.inl")).read()
    assert "constexpr uint32_t kDenseWindow = %d;" % W in src
    assert dc.DENSE_WINDOW == W


@pytest.mark.parametrize("k_type", [(1, False), (1, True), (2, True), (4, False), (4, True), (8, False), (8, True)],
                         ids=lambda t: "%s%d" % ("i" if t[1] else "u", 8 * t[0]))
def test_mirror_against_the_rule_in_python_integers(k_type):
    size, signed = k_type
    tb = 8 * size
    tmin, tmax = type_ends(size, signed)
    seen = set()
    for w in range(1, tb + 1):
        ext = (1 << w) - 1
        # frames: at the type's ends, around zero, one past the last that fits (wraps), none, unpacked
        firsts = {tmin, tmax - ext, tmax - ext + 1, 0, -1 if signed else 1, (tmin + tmax) // 2}
        descs = [seg(w, f) for f in sorted(firsts) if tmin <= f <= tmax]
        descs += [seg(w, None), seg(tb, 0, packed=False), seg(w, max(tmin, 0), count=0),
                  seg(w, max(tmin, 0), count=(1 << 31) // w + 1 if w <= 32 else 1000)]
        for d in descs:
            iv = interval(d, size, signed) or (tmin, tmax)
            for span in (1, W - 1, W, W + 1, 4 * W, 1 << 20):
                span = min(span, 1 << tb, 1 << 32)
                # the domain misses on either side, touches either end, sits inside, contains
                starts = {iv[0] - span, iv[0] - span + 1, iv[0], iv[0] + 1, iv[1], iv[1] + 1, iv[1] - span + 1,
                          (iv[0] + iv[1]) // 2, iv[0] - span // 2, tmin, tmax - span + 1}
                for lo in starts:
                    if lo < tmin or lo + span - 1 > tmax:
                        continue
                    base = lo & ((1 << tb) - 1)
                    got = forms.dense_form_groups(d, k_type, base, span)[0]
                    assert got == brute(d, k_type, base, span), (w, d, lo, span)
                    seen.add(got)
                    for dv, vt in ((seg(9, 5), (2, False)), (seg(40, 5), (8, True)), (seg(8, None), (1, True)),
                                   (seg(32, packed=False), (4, False)), (seg(1, 0xFF), (1, True))):
                        got = forms.dense_form_groups(d, k_type, base, span, dv, vt)[0]
                        assert got == brute(d, k_type, base, span, dv, vt), (w, d, lo, span, dv, vt)
                        seen.add(got)
    # (an 8- or 16-bit key reaches few indices past the window or none: the direct forms need the wider types)
    want = (set(dc.ALL_FORMS) if tb >= 32 else {"header", "walk-window", "staged-window"}) | {None}
    assert seen >= want, seen


def test_literals_worked_out_from_dense_plan():
    U32, I32, U64 = (4, False), (4, True), (8, False)
    f = lambda d, t, b, s, *v: forms.dense_form_groups(d, t, b, s, *v)[0]
    assert f(seg(8, 100), U32, 356, 10) == "header" and f(seg(8, 100), U32, 355, 1) == "walk-window"
    assert f(seg(13, 1000), U32, 1000, W) == "walk-window" and f(seg(13, 1000), U32, 1000, W + 1) == "walk-direct"
    assert f(seg(13, 1000), U32, 0, 1000 + W) == "walk-window"   # only the part from the frame on counts
    assert f(seg(9, 7), U32, 0, 1 << 32) == "walk-window" and f(seg(10, 7), U32, 0, 1 << 32) == "walk-direct"
    assert f(seg(3, 100), U32, 100, 4) == "staged-window" and f(seg(40, 0), U64, 10, 70000) == "staged-direct"
    assert f(seg(8, None), I32, 0, 300) == "staged-direct" and f(seg(8, None), U32, 256, 5) == "header"
    # the value column can take the walk away, never the window or the header
    assert f(seg(13, 1000), U32, 1000, W, seg(33, 0), U64) == "staged-window"
    assert f(seg(13, 1000), U32, 1000, W, seg(32, 0), U64) == "walk-window"
    assert f(seg(13, 1000), U32, 1000, W + 1, seg(8, None), I32) == "staged-direct"
    assert f(seg(13, 1000), U32, 1000, W + 1, seg(16, packed=False), (2, False)) == "walk-direct"
    assert f(seg(13, 1000), U32, 1000, W + 1, seg(16, packed=False), (2, True)) == "staged-direct"
    assert f(seg(13, 1000), U32, 1 << 20, 5, seg(40, 0), U64) == "header"
    assert f(seg(13, 1000), U32, 1000, 5, seg(8, 0, count=1 << 28), U32) == "staged-window"


def test_the_fuzz_draws_reach_every_form(oracle):
    seen, inside = set(), 0
    for seed in range(dc.FUZZ_SEEDS):
        rng, keys, vals, counts, rule, pad, base, span, combine = dc.fuzz_draw(seed)
        dk = sc.oracle_descs(oracle, adac, keys, counts, rule, pad)
        dv = sc.oracle_descs(oracle, adac, vals, counts, rule, pad)
        seen |= set(forms.dense_form_groups(dk, sm.kind(keys.dtype), base, span, dv, sm.kind(vals.dtype)))
        seen |= set(forms.dense_form_groups(dk, sm.kind(keys.dtype), base, span))
        inside += int(sm.member_index(keys, base, span)[1].sum())
    assert seen >= dc.ALL_FORMS, seen
    assert inside > 1000
