"""forms.mapped_product_form_groups (the host mirror of mapped_product_plan, csrc/adac_group_mapped_product.inl) against
the rule written once more with Python integers over the MATHEMATICAL values, and the columns of the GPU tests held on the
CPU: they reach every one of the five forms, and reach the staged form both because of `a` and because of `b`.  Without
this census the GPU tests could pass on columns that never leave one form.  mapped_form_groups and dense_form_groups
keep their signatures and results."""
import importlib
import inspect

import numpy as np
import pytest

import mapped_cases as mc
import product_mapped_cases as pc
import scan_compare_cases as sc
import scan_member_cases as sm
from test_group_dense_forms import as_value, interval, seg, type_ends
from test_group_mapped_forms import VALUE_SIDES, brute as mapped_brute

adac = importlib.import_module("duckdb-adaptive-compression_amd")
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")
S = forms.MAPPED_SLICE


def brute(d, k_type, base, span, da, a_type, db, b_type):
    """header: the key interval misses the domain; walk: key, a AND b walkable; slice: the reach alone"""
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
    walk = walkable(d, k_type, 4) and walkable(da, a_type, 1) and walkable(db, b_type, 1)
    return ("walk" if walk else "staged") + ("-slice" if reach <= S else "-direct")


# value columns: walkable ones, and one failing each clause of the rule (width, no frame, raw and signed, too many bits)
SIDES = VALUE_SIDES + ((seg(32, 7), (8, False)), (seg(33, 7), (8, False)), (seg(5, -40), (1, True)),
                       (seg(16, 0, count=(1 << 31) // 16), (4, False)), (seg(16, 0, count=(1 << 31) // 16 - 1), (4, False)))


@pytest.mark.parametrize("k_type", [(1, False), (2, True), (4, False), (4, True), (8, False), (8, True)],
                         ids=lambda t: "%s%d" % ("i" if t[1] else "u", 8 * t[0]))
def test_mirror_against_the_rule_in_python_integers(k_type):
    size, signed = k_type
    tb = 8 * size
    tmin, tmax = type_ends(size, signed)
    seen, staged_by = set(), set()
    for w in (1, 3, 4, 5, 11, 12, 13, 31, 32, 33, 64):
        if w > tb:
            continue
        ext = (1 << w) - 1
        firsts = {tmin, tmax - ext, tmax - ext + 1, 0, (tmin + tmax) // 2}
        descs = [seg(w, f) for f in sorted(firsts) if tmin <= f <= tmax]
        descs += [seg(w, None), seg(tb, 0, packed=False), seg(w, max(tmin, 0), count=0)]
        for d in descs:
            iv = interval(d, size, signed) or (tmin, tmax)
            for span in (1, S, S + 1, 1 << 20):
                span = min(span, 1 << tb, 1 << 32)
                for lo in {iv[0] - span, iv[0], iv[1], iv[1] + 1, (iv[0] + iv[1]) // 2, iv[1] - S + 1, iv[1] - S}:
                    if lo < tmin or lo + span - 1 > tmax:
                        continue
                    base = lo & ((1 << tb) - 1)
                    keys_only = forms.mapped_form_groups(d, k_type, base, span)[0]
                    alone = [forms.mapped_form_groups(d, k_type, base, span, dv, vt)[0] for dv, vt in SIDES]
                    for (da, at), one_a in zip(SIDES, alone):
                        for (db, bt), one_b in zip(SIDES, alone):
                            got = forms.mapped_product_form_groups(d, k_type, base, span, da, at, db, bt)[0]
                            assert got == brute(d, k_type, base, span, da, at, db, bt), (w, d, lo, span, da, at, db, bt)
                            seen.add(got)
                            # neither value column can take the slice or the header away, or give the walk back
                            if keys_only in (None, "header") or keys_only.startswith("staged"):
                                assert got == keys_only
                                continue
                            assert got.split("-")[1] == keys_only.split("-")[1]
                            if got.startswith("staged"):
                                staged_by.add(("a" if one_a.startswith("staged") else "") +
                                              ("b" if one_b.startswith("staged") else ""))
    want = (set(mc.ALL_FORMS) if tb >= 32 else {"header", "walk-slice", "staged-slice"}) | {None}
    assert seen >= want, seen
    assert staged_by == {"a", "b", "ab"}, staged_by


def test_literals_worked_out_from_mapped_product_plan():
    U32, I8, U64, I64 = (4, False), (1, True), (8, False), (8, True)
    f = lambda d, t, b, s, da, at, db, bt: forms.mapped_product_form_groups(d, t, b, s, da, at, db, bt)[0]
    key = seg(13, 1000)
    # a walkable, b at w = 33 -> staged; the converse; both at 32 -> walk
    assert f(key, U32, 1000, S, seg(24, 90000), I64, seg(33, 0), U64) == "staged-slice"
    assert f(key, U32, 1000, S, seg(33, 0), U64, seg(4, 0), I8) == "staged-slice"
    assert f(key, U32, 1000, S, seg(32, 0), U64, seg(32, 5), I64) == "walk-slice"
    assert f(key, U32, 1000, S + 1, seg(24, 90000), I64, seg(4, 0), I8) == "walk-direct"
    # b raw and signed (no frame), b with ADAC_NO_MIN, b past 2^31 bits
    assert f(key, U32, 1000, S + 1, seg(24, 90000), I64, seg(8, 0, packed=False), I8) == "staged-direct"
    assert f(key, U32, 1000, S, seg(24, 90000), I64, seg(8, None), I8) == "staged-slice"
    assert f(key, U32, 1000, S, seg(24, 90000), I64, seg(32, 0, count=1 << 26), U64) == "staged-slice"
    assert f(key, U32, 1000, S, seg(24, 90000), I64, seg(32, 0, count=(1 << 26) - 1), U64) == "walk-slice"
    # neither can take the slice or the header away
    assert f(key, U32, 1 << 20, 5, seg(40, 0), U64, seg(64, 0, packed=False), I64) == "header"
    assert f(key, U32, 1000, S, seg(40, 0), U64, seg(64, 0, packed=False), I64) == "staged-slice"
    assert f(key, U32, 1000, S + 1, seg(40, 0), U64, seg(64, 0, packed=False), I64) == "staged-direct"
    # the key side decides first: w = 3 and w = 40 are staged whatever the values are
    assert f(seg(3, 100), U32, 100, 4, seg(8, 0), U32, seg(8, 0), U32) == "staged-slice"
    assert f(seg(40, 0), U64, 10, 70000, seg(8, 0), U32, seg(8, 0), U32) == "staged-direct"
    # a == b, and a == keys
    assert f(key, U32, 1000, S, key, U32, key, U32) == "walk-slice"
    assert f(seg(3, 100), U32, 100, 4, seg(3, 100), U32, seg(3, 100), U32) == "staged-slice"


def test_the_older_mirrors_keep_their_signatures_and_results():
    assert list(inspect.signature(forms.mapped_form_groups).parameters) == \
        ["descs_k", "k_type", "key_base", "key_span", "descs_v", "v_type"]
    assert list(inspect.signature(forms.dense_form_groups).parameters) == \
        ["descs_k", "k_type", "key_base", "key_span", "descs_v", "v_type"]
    assert list(inspect.signature(forms.mapped_product_form_groups).parameters) == \
        ["descs_k", "k_type", "key_base", "key_span", "descs_a", "a_type", "descs_b", "b_type"]
    for k_type in ((4, False), (8, True)):
        tmin, tmax = type_ends(*k_type)
        for w in (3, 11, 12, 33):
            for d in (seg(w, 0), seg(w, tmin), seg(w, None)):
                iv = interval(d, *k_type) or (tmin, tmax)
                for span in (1, S, S + 1):
                    for lo in (iv[0], iv[1], iv[0] - span + 1):
                        if lo < tmin or lo + span - 1 > tmax:
                            continue
                        base = lo & ((1 << (8 * k_type[0])) - 1)
                        assert forms.mapped_form_groups(d, k_type, base, span)[0] == mapped_brute(d, k_type, base, span)
                        for dv, vt in VALUE_SIDES:
                            assert (forms.mapped_form_groups(d, k_type, base, span, dv, vt)[0]
                                    == mapped_brute(d, k_type, base, span, dv, vt))
                            # with the same column on both sides the product rule is the pair rule
                            assert (forms.mapped_product_form_groups(d, k_type, base, span, dv, vt, dv, vt)
                                    == forms.mapped_form_groups(d, k_type, base, span, dv, vt))


def test_the_gpu_tests_columns_reach_every_form(oracle):
    """the fuzz's fixed seeds, the key width grid and the value-width columns of test_gpu_group_product_mapped*.py"""
    seen, why, inside = set(), set(), 0

    def note(keys, a, b, counts, rule, pad, base, span):
        dk = sc.oracle_descs(oracle, adac, keys, counts, rule, pad)
        da = sc.oracle_descs(oracle, adac, a, counts, rule, pad)
        db = sc.oracle_descs(oracle, adac, b, counts, rule, pad)
        kt, at, bt = sm.kind(keys.dtype), sm.kind(a.dtype), sm.kind(b.dtype)
        got = forms.mapped_product_form_groups(dk, kt, base, span, da, at, db, bt)
        only_a = forms.mapped_form_groups(dk, kt, base, span, da, at)
        only_b = forms.mapped_form_groups(dk, kt, base, span, db, bt)
        for f, k, fa, fb in zip(got, forms.mapped_form_groups(dk, kt, base, span), only_a, only_b):
            if f is not None and f.startswith("staged") and k.startswith("walk"):
                why.add(("a" if fa.startswith("staged") else "") + ("b" if fb.startswith("staged") else ""))
        return set(got)

    for seed in range(mc.FUZZ_SEEDS):
        rng, keys, a, b, counts, rule, pad, base, span, knob, ngroups, codes = pc.fuzz_draw(seed)
        assert len(b) == len(a) == len(keys) and len(codes) == span
        drawn = mc.fuzz_draw(seed)   # b's generator leaves the older draws what they are
        assert np.array_equal(drawn[1], keys) and np.array_equal(drawn[2], a) and np.array_equal(drawn[10], codes)
        seen |= note(keys, a, b, counts, rule, pad, base, span)
        inside += int(sm.member_index(keys, base, span)[1].sum())
    assert seen >= mc.ALL_FORMS, seen
    assert inside > 1000
    for dtype in sm.GRID_TYPES:
        dtype = np.dtype(dtype)
        keys, a, b, doms = pc.key_width_grid(dtype)
        counts = np.full(8 * dtype.itemsize, sm.ROWS_GRID, dtype=np.uint32)
        grid = set()
        for base, span in doms:
            grid |= note(keys, a, b, counts, 0, False, base, span)
        # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 indices: no staged reader without a slice)
        assert grid >= mc.ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), (dtype, grid)
    counts = np.full(pc.VW_SEGS, pc.VW_ROWS, dtype=np.uint32)
    for vtype in (np.uint64, np.int64):
        keys, sweep, cyc, _ = pc.value_width_columns(vtype)
        for x, y in ((sweep, cyc), (cyc, sweep)):
            got = forms.mapped_product_form_groups(sc.oracle_descs(oracle, adac, keys, counts), (4, False), 1200, S,
                                                   sc.oracle_descs(oracle, adac, x, counts), sm.kind(vtype),
                                                   sc.oracle_descs(oracle, adac, y, counts), sm.kind(vtype))
            assert got == ["walk-slice"] * 32 + ["staged-slice"] * 32
            note(keys, x, y, counts, 0, False, 1200, S)
    assert {"a", "b"} <= why, why
