"""The columns the GPU tests of the member scans run on, held on the CPU: forms.member_form_groups (the host mirror of
member_plan, csrc/adac_scan_member.inl) on hand-made descriptors, the reference of scan_member_cases.py against Python
integers, and the width grid: its widths by the reference's width rule, all four row classes in every segment, all five
kernel forms.  Without this the GPU tests could pass on columns that never meet their domain or never leave one form."""
import importlib

import numpy as np
import pytest

import scan_compare_cases as sc
import scan_member_cases as sm

adac = importlib.import_module("duckdb-adaptive-compression_amd")
forms = importlib.import_module("duckdb-adaptive-compression_amd.forms")

NO_MIN = 0xFFFFFFFFFFFFFFFF
U32, I32, U64 = (4, False), (4, True), (8, False)
ALL_FORMS = {"header", "walk-slice", "walk-direct", "staged-slice", "staged-direct"}


def seg(width, vmin=0, count=1000, packed=True):
    d = np.zeros(1, dtype=adac.SEGMENT_DESC_DTYPE)
    d["count"], d["width"], d["flags"] = count, width, 1 if packed else 0
    d["min"] = NO_MIN if vmin is None else vmin & NO_MIN
    return d


def form(d, type, base, bits):
    return forms.member_form_groups(d, type, base, bits)[0]


def test_the_rule_at_its_boundaries():
    """literals worked out from member_plan"""
    assert form(seg(8, 100), U32, 356, 10) == "header"               # [100, 355] below the domain
    assert form(seg(8, 100), U32, 355, 1) == "walk-slice"            # touching
    assert form(seg(8, 100), U32, 0, 100) == "header" and form(seg(8, 100), U32, 0, 101) == "walk-slice"
    assert form(seg(3, 100), U32, 100, 4) == "staged-slice"          # w < 4
    assert form(seg(3, 100), U32, 108, 4) == "header"                # the header form has no width bound
    assert form(seg(40, 0), U64, 10, 1000) == "staged-slice"         # w > 32, a small domain inside the interval
    assert form(seg(40, 0), U64, 10, 70000) == "staged-direct"
    assert form(seg(40, 0), U64, 1 << 40, 70000) == "header"
    assert form(seg(8, None), I32, 0, 300) == "staged-direct"        # int32 without a stored min: no frame
    assert form(seg(8, None), U32, 256, 5) == "header"               # uint32: [0, 255]
    assert form(seg(8, None), U32, 255, 5) == "walk-slice"
    assert form(seg(32, packed=False), U32, 7, 100) == "walk-slice"  # raw unsigned slots: the whole type, 100 bits reached
    assert form(seg(32, packed=False), U32, 7, 1 << 20) == "walk-direct"
    assert form(seg(32, packed=False), I32, 7, 100) == "staged-direct"
    assert form(seg(4, (1 << 31) - 15), I32, 0, 100) == "staged-direct"   # the frame leaves int32
    # int32 -5 ... 10
    assert form(seg(4, 0xFFFFFFFB), I32, 0xFFFFFFFD, 10) == "walk-slice"  # from -3
    assert form(seg(4, 0xFFFFFFFB), I32, 11, 50) == "header"
    assert form(seg(4, 0xFFFFFFFB), I32, sm.pattern(np.int32, -100), 95) == "header"        # -100 ... -6
    assert form(seg(4, 0xFFFFFFFB), I32, sm.pattern(np.int32, -100), 96) == "walk-slice"    # ... -5
    assert form(seg(4, 0xFFFFFFFB), I32, 1 << 31, 1 << 32) == "walk-slice"                  # the whole type
    # uint64 at the top of the type
    assert form(seg(4, NO_MIN - 16), U64, NO_MIN - 3, 4) == "walk-slice"
    assert form(seg(4, NO_MIN - 40), U64, NO_MIN - 3, 4) == "header"
    assert form(seg(32, 0, count=1 << 26), U32, 0, 10) == "staged-slice"  # 2^31 bits: not the walk
    assert forms.member_form_groups(seg(8, 1, count=0), U32, 0, 10) == [None]


def test_the_slice_boundary():
    """the set bits a segment's interval can reach: 65536 is a slice, 65537 is not; w = 16 always is"""
    assert form(seg(20, 0), U32, 0, 65536) == "walk-slice" and form(seg(20, 0), U32, 0, 65537) == "walk-direct"
    assert form(seg(20, 0), U32, 5, 65536) == "walk-slice" and form(seg(20, 0), U32, 5, 65537) == "walk-direct"
    # the domain begins before the interval: only the part from the frame on counts
    assert form(seg(20, 1000), U32, 0, 1000 + 65536) == "walk-slice"
    assert form(seg(20, 1000), U32, 0, 1000 + 65537) == "walk-direct"
    # the domain ends after the interval: only the part up to frame + 2^w - 1 counts
    top = 1000 + (1 << 20)
    assert form(seg(20, 1000), U32, top - 65536, 1 << 24) == "walk-slice"
    assert form(seg(20, 1000), U32, top - 65537, 1 << 24) == "walk-direct"
    assert form(seg(40, 0), U64, 77, 65536) == "staged-slice" and form(seg(40, 0), U64, 77, 65537) == "staged-direct"
    for base, bits in ((0, 1 << 32), (1000, 1 << 24), (999, 65537), (1031, 1 << 20)):
        assert form(seg(16, 1000), U32, base, bits) == "walk-slice", (base, bits)
        assert form(seg(17, 1000), U32, base, max(bits, 1 << 18)) == "walk-direct", (base, bits)
    for w in range(1, 17):
        assert form(seg(w, 31), U32, 0, 1 << 32).endswith("-slice"), w


def test_the_reference_is_exact_for_every_type():
    """member_index / member_mask / built_set against Python integers over the mathematical values"""
    rng = np.random.default_rng(2000)
    for t in sm.TYPES:
        dtype = np.dtype(t)
        vals = sc.typed_column(t)
        pv = [int(x) for x in vals]
        info = np.iinfo(dtype)
        for name, base, bits in sm.typed_domains(dtype):
            lo = base - (1 << (8 * dtype.itemsize)) if base > info.max else base   # the pattern as a value of the type
            assert info.min <= lo and lo + bits - 1 <= info.max, (t, name)
            words = sm.random_set(rng, bits, 0.5)
            tix, inside = sm.member_index(vals, base, bits)
            assert inside.tolist() == [lo <= x <= lo + bits - 1 for x in pv], (t, name)
            assert all(int(ti) == x - lo for ti, x, i in zip(tix, pv, inside) if i), (t, name)
            exp = [lo <= x <= lo + bits - 1 and bool((int(words[(x - lo) >> 6]) >> ((x - lo) & 63)) & 1) for x in pv]
            assert sm.member_mask(vals, base, bits, words).tolist() == exp, (t, name)
            built, ins = sm.built_set(vals, base, bits)
            want = np.zeros(len(built) * 64, dtype=bool)
            want[[x - lo for x in pv if lo <= x <= lo + bits - 1]] = True
            assert np.array_equal(np.unpackbits(built.view(np.uint8), bitorder="little").astype(bool), want), (t, name)
            assert ins.tolist() == inside.tolist()
        # every type has rows at its ends, and the domains at the ends select some
        assert info.min in pv and info.max in pv


def test_tail_bits_of_a_random_set_are_set():
    rng = np.random.default_rng(2001)
    for bits in (1, 2, 63, 65, 100, 65537):
        w = sm.random_set(rng, bits, 0.0)
        b = np.unpackbits(w.view(np.uint8), bitorder="little")
        assert not b[:bits].any() and b[bits:].all() and (bits % 64 == 0 or b[bits:].any())


@pytest.mark.parametrize("dtype", sm.GRID_TYPES, ids=lambda t: np.dtype(t).name)
def test_width_grid_reaches_its_widths_and_all_four_classes(oracle, dtype):
    dtype = np.dtype(dtype)
    vals, doms = sm.width_grid(dtype)
    nseg = 8 * dtype.itemsize
    counts = np.full(nseg, sm.ROWS_GRID, dtype=np.uint32)
    d = sc.oracle_descs(oracle, adac, vals, counts)
    assert [int(x) for x in d["width"]] == list(range(1, nseg + 1))
    seen = set()
    for s, (base, bits, words) in enumerate(doms):
        assert 1 <= bits <= 1 << 24 and len(words) == sm.set_words_for(bits)
        f = forms.member_form_groups(d, sm.kind(dtype), base, bits)
        assert f[s] not in (None, "header"), (s, f[s])
        seen |= set(f)
        got = sm.classes_of(vals[s * sm.ROWS_GRID:(s + 1) * sm.ROWS_GRID], base, bits, words)
        if s == 0:   # one bit: two values
            assert got["set"] and got["clear"], got
        else:
            assert all(got.values()), (s + 1, got)
        if bits % 64:
            assert int(words[-1]) >> (bits % 64) == (1 << (64 - bits % 64)) - 1   # the tail is set
    # (a uint32 segment always has a frame and at w <= 3 reaches at most 8 bits: no staged reader with direct access)
    assert seen == ALL_FORMS - ({"staged-direct"} if dtype == np.uint32 else set()), seen
    if dtype.kind == "i":
        assert (vals < 0).any() and (vals > 0).any()


def test_the_fuzz_draws_reach_every_form_and_select_rows(oracle):
    from test_gpu_scan_member_fuzz import SEEDS, draw
    seen, selected, inside = set(), 0, 0
    for seed in range(SEEDS):
        rng, dtype, counts, vals, rule, pad, base, bits, density = draw(seed)
        d = sc.oracle_descs(oracle, adac, vals, counts, rule, pad)
        seen |= set(forms.member_form_groups(d, sm.kind(dtype), base, bits))
        words = sm.random_set(rng, bits, density)
        selected += int(sm.member_mask(vals, base, bits, words).sum())
        inside += int(sm.member_index(vals, base, bits)[1].sum())
    assert seen >= ALL_FORMS, seen
    assert selected > 1000 and inside > selected
