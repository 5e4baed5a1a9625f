"""What the seed lists of tests/test_gpu_bitpacking_scans_fuzz.py reach, asserted on the CPU from the block images the
oracle wrote (mode, width, frame and step of every metadata group): a seed list that stops reaching a decision edge
fails here, without a GPU.  The figures are conditions on the generator (tests/bp_fuzz_columns.py), not measurements.

One condition is read in the only way the codec allows.  "A CONSTANT_DELTA group whose last row wraps T" cannot exist
in an encoded column in the arithmetic sense: a signed run that passes T's maximum has a delta outside T_S (or max - min
outside it), an unsigned one has a maximum above T_S's, and Flush takes neither as a delta mode
(test_a_run_that_wraps_the_type_is_never_constant_delta).  What does exist, and what the scans' first + row * step on
unsigned bit patterns has to get right, is a linear form that passes 2^bits on those bit patterns by the last row: every
unsigned run with a negative step (the step is 2^bits - |step|), and a signed run with a positive step that crosses
from negative to non-negative.  Those are asserted."""
import collections

import numpy as np
import pytest

import bp_fuzz_columns as fz
from bp_pair_cases import GROUP, Packed
from oracle import bitpacking as bp

C, CD, DF, FOR = bp.MODE_CONSTANT, bp.MODE_CONSTANT_DELTA, bp.MODE_DELTA_FOR, bp.MODE_FOR


def signed_of(x, bits):
    return x - (1 << bits) if x >> (bits - 1) else x


class Census:
    def __init__(self):
        self.delta64 = collections.Counter()        # width class of 64-bit DELTA_FOR -> groups
        self.delta64_desc = collections.Counter()   # the descending ones among them
        self.cd = collections.Counter()             # (signed type, what) -> CONSTANT_DELTA groups
        self.full_width = collections.Counter()     # item size -> FOR / DELTA_FOR groups at the type's full width
        self.null_columns = self.all_null_group = 0
        self.draws = collections.Counter()

    def column(self, col):
        bits = 8 * col.dtype.itemsize
        sg = col.dtype.kind == "i"
        self.draws[col.draws] += 1
        if col.validity is not None:
            self.null_columns += 1
            n = len(col.validity)
            self.all_null_group += any(not col.validity[g:g + GROUP].any() for g in range(0, n, GROUP))
        groups = fz.segment_groups(col.comp)
        row = 0
        for _, _, rows, mode, width, frame, extra in groups:
            if mode == DF and bits == 64:
                cls = "<=26" if width <= 26 else "27-32" if width <= 32 else ">32"
                self.delta64[cls] += 1
                steps = np.diff(col.values[row:row + rows].view(np.int64))    # (a delta group's deltas fit T_S)
                self.delta64_desc[cls] += bool((steps <= 0).all() and (steps < 0).any() and signed_of(frame, bits) < 0)
            row += rows
            if mode == CD:
                step = signed_of(extra, bits)
                self.cd[(sg, "negative")] += step < 0
                self.cd[(sg, "carries")] += frame + (rows - 1) * extra >= 1 << bits and (step > 0 or not sg)
            if mode in (DF, FOR) and width == bits:
                self.full_width[bits // 8] += 1
        return groups


@pytest.fixture(scope="module")
def census():
    cs = Census()
    cs.single_n, cs.pair_n = set(), set()
    cs.combos = collections.Counter()
    cs.delta_side_under_steps = collections.Counter()
    cs.segments_differ = 0
    for seed in fz.SINGLE_SEEDS:
        c = fz.single_case(seed)
        cs.single_n.add(c.n)
        cs.column(c.col)
    for seed in fz.PAIR_SEEDS:
        c = fz.pair_case(seed)
        cs.pair_n.add(c.n)
        ga, gb = cs.column(c.a), cs.column(c.b)
        assert len(ga) == len(gb)
        cs.segments_differ += c.a.comp.nseg != c.b.comp.nseg
        steps = c.masks["steps"][c.phase:c.phase + c.n]
        for g, (x, y) in enumerate(zip(ga, gb)):
            cs.combos[(x[3], y[3])] += 1
            st = steps[g * GROUP:(g + 1) * GROUP:64]
            if ((x[3] == DF and x[4] >= 1) or (y[3] == DF and y[4] >= 1)) and not st.all() and st[np.argmin(st):].any():
                cs.delta_side_under_steps[(x[3], y[3])] += 1
    print("\nmode pairs:", sorted(cs.combos.items()))
    print("pairs with a DELTA_FOR side under a clear-then-set steps mask:", sorted(cs.delta_side_under_steps.items()))
    print("pair seeds whose segment counts differ:", cs.segments_differ)
    print("64-bit DELTA_FOR groups by width:", dict(cs.delta64), "descending:", dict(cs.delta64_desc))
    print("CONSTANT_DELTA (signed type, what):", dict(cs.cd))
    print("full-width FOR / DELTA_FOR groups by item size:", dict(cs.full_width))
    print("columns under a NULL mask:", cs.null_columns, "with an all-NULL group:", cs.all_null_group)
    print("draws needed per column:", dict(cs.draws))
    return cs


def test_pair_seeds_reach_every_mode_pair(census):
    for a in (C, CD, DF, FOR):
        for b in (C, CD, DF, FOR):
            assert census.combos[(a, b)] >= 4, (a, b, census.combos[(a, b)])
            if DF in (a, b):
                assert census.delta_side_under_steps[(a, b)] >= 2, (a, b)
    assert census.segments_differ >= 6


def test_delta_for_of_64_bit_types_in_every_width_class(census):
    for cls in ("<=26", "27-32", ">32"):
        assert census.delta64[cls] >= 4, (cls, census.delta64)
        assert census.delta64_desc[cls] >= 1, (cls, census.delta64_desc)


def test_constant_delta_steps(census):
    for sg in (False, True):
        assert census.cd[(sg, "negative")] >= 1, census.cd
        assert census.cd[(sg, "carries")] >= 1, census.cd


def test_full_width_and_null_masks(census):
    for ts in (1, 2, 4, 8):
        assert census.full_width[ts] >= 1, census.full_width
    assert sum(census.full_width.values()) >= 10
    assert census.null_columns >= 12 and census.all_null_group >= 3


def test_every_length(census):
    assert census.single_n >= set(fz.FIXED_N) and census.pair_n >= set(fz.FIXED_N)
    for ns in (census.single_n, census.pair_n):
        assert any(n < 9000 and n not in fz.FIXED_N for n in ns) and any(9000 <= n < 30000 for n in ns)
        assert any(30000 <= n < 80000 for n in ns)


def test_no_column_needed_a_ninth_draw(census):
    assert max(census.draws) <= fz.MAX_DRAWS - 1, census.draws


def test_group_headers_agree_with_group_info():
    """segment_groups reads mode and width as the oracle's own group_info does"""
    seed = next(s for s in fz.PAIR_SEEDS if s % 14 == 13 and s % fz.MULTI_EVERY != fz.MULTI_AT)   # a long column
    for col in fz.pair_columns(seed):
        assert len(col.values) >= 30000
        groups = fz.segment_groups(col.comp)
        assert [(m, w) for _, _, _, m, w, _, _ in groups] == Packed(col.values, col.force, validity=col.validity).modes


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.int64, np.uint16, np.uint32, np.uint64])
@pytest.mark.parametrize("step", [3, -3])
def test_a_run_that_wraps_the_type_is_never_constant_delta(dtype, step):
    """first + row * step passing T's maximum (or minimum) at the last row: FOR, or refused, never a delta mode"""
    dtype = np.dtype(dtype)
    info = np.iinfo(dtype)
    first = (int(info.max) - 3 * 2046) if step > 0 else (int(info.min) + 3 * 2046)
    v = np.array([(first + step * i) & fz.M64 for i in range(GROUP)], dtype=np.uint64)
    v = v.astype("u%d" % dtype.itemsize).view(dtype)
    assert (int(v[-1]) < int(v[-2])) == (step > 0)           # the last row wrapped
    for force in (bp.MODE_AUTO, bp.MODE_CONSTANT_DELTA, bp.MODE_DELTA_FOR):
        try:
            comp = bp.Compressed(v, force_mode=force)
        except ValueError:
            continue
        assert comp.groups_by_mode()["constant_delta"] == 0 and comp.groups_by_mode()["delta_for"] == 0
