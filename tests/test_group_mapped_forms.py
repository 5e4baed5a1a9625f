"""forms.mapped_form_groups (the host mirror of mapped_plan, csrc/adac_group_mapped.inl) against the rule written once
more with Python integers over the MATHEMATICAL values, and the columns of the GPU tests held on the CPU: the fuzz's fixed
seeds and the width grid reach every one of the five forms.  Without this census the GPU tests could pass on columns
that never leave one form.  dense_form_groups, which shares the helper, keeps its results."""
import importlib
import os
import re

import numpy as np
import pytest

import dense_cases as dc
import mapped_cases as mc
import scan_compare_cases as sc
import scan_member_cases as sm
from test_group_dense_forms import as_value, brute as dense_brute, interval, seg, type_ends

adac = importlib.import_module("duckdb-adaptive-compression_amd")
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = forms.MAPPED_SLICE


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
    return ("walk" if walk else "staged") + ("-slice" if reach <= S else "-direct")


def test_the_slice_is_the_kernels():
    src = open(os.path.join(ROOT, "duckdb-adaptive-compression_amd", "csrc", "adac_group_mapped.inl")).read()
    m = re.search(r"constexpr uint32_t kMappedSlice = (\d+);", src)
    assert m and int(m.group(1)) == S == mc.MAPPED_SLICE
    assert S & (S - 1) == 0


VALUE_SIDES = ((seg(9, 5), (2, False)), (seg(40, 5), (8, True)), (seg(8, None), (1, True)),
               (seg(32, packed=False), (4, False)), (seg(1, 0xFF), (1, True)))


@pytest.mark.parametrize("k_type", [(1, False), (1, True), (2, True), (4, False), (4, True), (8, False), (8, True)],
                         ids=lambda t: "%s%d" % ("i" if t[1] else "u", 8 * t[0]))
def test_mirror_against_the_rule_in_python_integers(k_type):
    size, signed = k_type
    tb = 8 * size
    tmin, tmax = type_ends(size, signed)
    seen = set()
    for w in range(1, tb + 1):
        ext = (1 << w) - 1
        # frames: at the type's ends (the signed types' too), around zero, one past the last that fits (wraps), none,
        # unpacked
        firsts = {tmin, tmax - ext, tmax - ext + 1, 0, -1 if signed else 1, (tmin + tmax) // 2}
        descs = [seg(w, f) for f in sorted(firsts) if tmin <= f <= tmax]
        descs += [seg(w, None), seg(tb, 0, packed=False), seg(w, max(tmin, 0), count=0),
                  seg(w, max(tmin, 0), count=(1 << 31) // w + 1 if w <= 32 else 1000)]
        for d in descs:
            iv = interval(d, size, signed) or (tmin, tmax)
            for span in (1, S - 1, S, S + 1, 4 * S, 1 << 20):
                span = min(span, 1 << tb, 1 << 32)
                # the domain misses on either side, touches either end, sits inside, contains; reach = S and S + 1
                starts = {iv[0] - span, iv[0] - span + 1, iv[0], iv[0] + 1, iv[1], iv[1] + 1, iv[1] - span + 1,
                          (iv[0] + iv[1]) // 2, iv[0] - span // 2, tmin, tmax - span + 1, iv[1] - S + 1, iv[1] - S,
                          iv[0] - span + S, iv[0] - span + S + 1}
                for lo in starts:
                    if lo < tmin or lo + span - 1 > tmax:
                        continue
                    base = lo & ((1 << tb) - 1)
                    got = forms.mapped_form_groups(d, k_type, base, span)[0]
                    assert got == brute(d, k_type, base, span), (w, d, lo, span)
                    seen.add(got)
                    for dv, vt in VALUE_SIDES:
                        got = forms.mapped_form_groups(d, k_type, base, span, dv, vt)[0]
                        assert got == brute(d, k_type, base, span, dv, vt), (w, d, lo, span, dv, vt)
                        seen.add(got)
    # (an 8-bit key reaches at most 256 indices: the direct forms need the wider types)
    want = (set(mc.ALL_FORMS) if tb >= 16 else {"header", "walk-slice", "staged-slice"}) | {None}
    if tb == 16:
        want -= {"staged-direct"} if not signed else set()
    assert seen >= want, seen


def test_literals_worked_out_from_mapped_plan():
    U32, I32, U64 = (4, False), (4, True), (8, False)
    f = lambda d, t, b, s, *v: forms.mapped_form_groups(d, t, b, s, *v)[0]
    assert f(seg(8, 100), U32, 356, 10) == "header" and f(seg(8, 100), U32, 355, 1) == "walk-slice"
    # reach = MAPPED_SLICE and MAPPED_SLICE + 1
    assert f(seg(13, 1000), U32, 1000, S) == "walk-slice" and f(seg(13, 1000), U32, 1000, S + 1) == "walk-direct"
    assert f(seg(13, 1000), U32, 0, 1000 + S) == "walk-slice"   # only the part from the frame on counts
    assert f(seg(13, 1000), U32, 0, 1000 + S + 1) == "walk-direct"
    assert f(seg(11, 7), U32, 0, 1 << 32) == "walk-slice" and f(seg(12, 7), U32, 0, 1 << 32) == "walk-direct"
    assert f(seg(3, 100), U32, 100, 4) == "staged-slice" and f(seg(40, 0), U64, 10, 70000) == "staged-direct"
    assert f(seg(8, None), I32, 0, 300) == "staged-direct" and f(seg(8, None), U32, 256, 5) == "header"
    # signed keys at the type's ends
    i32min, i32max = 0x80000000, 0x7FFFFFFF
    assert f(seg(12, i32min), I32, i32min, S) == "walk-slice" and f(seg(12, i32min), I32, i32min, S + 1) == "walk-direct"
    assert f(seg(12, i32max - 4095), I32, i32max - S + 1, S) == "walk-slice"
    assert f(seg(12, i32max - 4095), I32, i32max - S, S + 1) == "walk-direct"
    assert f(seg(12, i32max - 4094), I32, i32max - 9, 10) == "staged-direct"   # the frame wraps: no interval
    assert f(seg(12, i32min), I32, 0, 10) == "header"
    # the value column can take the walk away, never the slice or the header
    assert f(seg(13, 1000), U32, 1000, S, seg(33, 0), U64) == "staged-slice"
    assert f(seg(13, 1000), U32, 1000, S, seg(32, 0), U64) == "walk-slice"
    assert f(seg(13, 1000), U32, 1000, S + 1, seg(8, None), I32) == "staged-direct"
    assert f(seg(13, 1000), U32, 1 << 20, 5, seg(40, 0), U64) == "header"


def test_dense_form_groups_is_unchanged():
    """the shared helper under its first caller: the dense rule in Python integers, on both sides of BOTH constants"""
    for k_type in ((4, False), (4, True), (8, True)):
        tmin, tmax = type_ends(*k_type)
        for w in (3, 9, 10, 11, 12, 20, 33):
            for d in (seg(w, 0), seg(w, tmin), seg(w, None), seg(8 * k_type[0], 0, packed=False)):
                iv = interval(d, *k_type) or (tmin, tmax)
                for span in (1, forms.DENSE_WINDOW, forms.DENSE_WINDOW + 1, S, S + 1, 1 << 20):
                    for lo in (iv[0], iv[0] + 1, iv[0] - span + 1, iv[1], (iv[0] + iv[1]) // 2):
                        if lo < tmin or lo + span - 1 > tmax:
                            continue
                        base = lo & ((1 << (8 * k_type[0])) - 1)
                        assert forms.dense_form_groups(d, k_type, base, span)[0] == dense_brute(d, k_type, base, span)
                        for dv, vt in VALUE_SIDES:
                            assert (forms.dense_form_groups(d, k_type, base, span, dv, vt)[0]
                                    == dense_brute(d, k_type, base, span, dv, vt))


def test_the_fuzz_draws_and_the_width_grid_reach_every_form(oracle):
    seen, inside, ngroups_seen, shapes = set(), 0, set(), 0
    for seed in range(mc.FUZZ_SEEDS):
        rng, keys, vals, counts, rule, pad, base, span, knob, ngroups, codes = mc.fuzz_draw(seed)
        dk = sc.oracle_descs(oracle, adac, keys, counts, rule, pad)
        dv = sc.oracle_descs(oracle, adac, vals, counts, rule, pad)
        seen |= set(forms.mapped_form_groups(dk, sm.kind(keys.dtype), base, span, dv, sm.kind(vals.dtype)))
        seen |= set(forms.mapped_form_groups(dk, sm.kind(keys.dtype), base, span))
        inside += int(sm.member_index(keys, base, span)[1].sum())
        ngroups_seen.add(ngroups)
        assert len(codes) == span and 1 <= ngroups <= 256
    assert seen >= mc.ALL_FORMS, seen
    assert inside > 1000 and len(ngroups_seen) >= 6
    for dtype in sm.GRID_TYPES:
        dtype = np.dtype(dtype)
        keys, vals, doms = mc.key_width_grid(dtype)
        nseg = 8 * dtype.itemsize
        counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
        dk = sc.oracle_descs(oracle, adac, keys, counts, 0, False)
        dv = sc.oracle_descs(oracle, adac, vals, counts, 0, False)
        grid = set()
        for base, span in doms:
            grid |= set(forms.mapped_form_groups(dk, sm.kind(dtype), base, span, dv, sm.kind(vals.dtype)))
        # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 indices: no staged reader without a slice)
        assert grid >= mc.ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), (dtype, grid)
